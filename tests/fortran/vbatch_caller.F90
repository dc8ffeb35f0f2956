!> Fortran caller of eigen_s_vbatch (an extension: the reference solves one matrix per call) on Frank blocks
!! (benchmark/mat_set.f:638-647) of the orders 7, 30, 70 and 12, scaled by 1, 2, 3 and 4, packed into flat arrays with padded
!! columns and gaps; the eigenvalues are known in closed form.  The start indices are 1-based.  The last block of a second call
!! carries a NaN and must fail alone; the guards between the blocks must survive both calls.
program vbatch_caller
  use eigen_libs_mod
  implicit none
  integer, parameter :: nb = 4, gap = 5
  integer :: n(nb), lda(nb), ldz(nb), info(nb), i, j, k, pass
  integer(8) :: ia(nb), iw(nb), iz(nb), ta, tw, tz, p
  real(8), allocatable :: a(:), z(:), w(:)
  logical, allocatable :: wmine(:)
  real(8) :: lam, err, pi, nan
  real(8), parameter :: guard = -7.25d0
  n = (/7, 30, 70, 12/)
  lda = n + 3
  ldz = n + 1
  ta = 1; tw = 1; tz = 1
  do k = 1, nb
    ia(k) = ta + gap; ta = ia(k) + int(lda(k), 8) * n(k)
    iw(k) = tw + gap; tw = iw(k) + n(k)
    iz(k) = tz + gap; tz = iz(k) + int(ldz(k), 8) * n(k)
  end do
  allocate(a(ta + gap), w(tw + gap), z(tz + gap), wmine(tw + gap))
  call eigen_init()
  pi = 4d0 * atan(1d0)
  nan = 0d0
  nan = nan / nan
  err = 0d0
  do pass = 1, 2
    a = nan
    do k = 1, nb
      do j = 1, n(k)
        do i = 1, j
          a(ia(k) + (i - 1) + int(lda(k), 8) * (j - 1)) = dble(k) * dble(min(i, j))
        end do
      end do
    end do
    info = 77
    w = guard
    z = guard
    if (pass == 1) then
      call eigen_s_vbatch(nb, n, a, ia, lda, w, iw, z, iz, ldz)
    else
      a(ia(nb) + 2 + int(lda(nb), 8) * 6) = nan
      call eigen_s_vbatch(nb, n, a, ia, lda, w, iw, z, iz, ldz, mode='N', info=info)
      if (any(info(1:nb - 1) /= 0) .or. info(nb) /= -5 .or. w(iw(nb)) == w(iw(nb))) then
        print *, "eigen_s_vbatch: wrong per-block status", info
        stop 1
      end if
      if (any(z /= guard)) then
        print *, "eigen_s_vbatch: mode N wrote z"
        stop 1
      end if
    end if
    wmine = .false.
    do k = 1, nb
      wmine(iw(k) : iw(k) + n(k) - 1) = .true.
    end do
    if (any(.not. wmine .and. w /= guard)) then
      print *, "eigen_s_vbatch: w was written between the blocks"
      stop 1
    end if
    if (pass == 1) then
      do k = 1, nb
        do j = 1, n(k)
          p = iz(k) + int(ldz(k), 8) * (j - 1)
          if (z(p + n(k)) /= guard .or. abs(sum(z(p : p + n(k) - 1)**2) - 1d0) > 1d-12) then
            print *, "eigen_s_vbatch: a padding row of z was written or a column is not normalised", k, j
            stop 1
          end if
        end do
      end do
    end if
    do k = 1, merge(nb, nb - 1, pass == 1)
      do j = 1, n(k)
        lam = dble(k) / (2d0 * (1d0 - cos((2 * (n(k) - j + 1) - 1) * pi / (2 * n(k) + 1))))
        err = max(err, abs(w(iw(k) + j - 1) - lam) / lam)
      end do
    end do
  end do
  print *, "eigen_s_vbatch max rel eigenvalue error =", err
  call eigen_free()
end program vbatch_caller
