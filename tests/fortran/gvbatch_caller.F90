!> Fortran caller of eigen_gev_vbatch (an extension: the reference solves one pencil per call) on pencils of the orders 7, 30, 70
!! and 12 packed into flat arrays with padded columns and gaps: A = the Frank matrix (benchmark/mat_set.f:638-647) scaled by
!! 1 .. 4, B = H^T diag(s) H with H the Helmert matrix of the block's order and s(i) = k + i / n.  The start indices are 1-based.
!! Prints, worst over the pencils and in units of the gate, ||A Z - B Z W||_F / (1e-12 scale n), ||Z^T B Z - I||_F / (1e-12 n)
!! and ||U^T U - B||_F / (1e-12 n ||B||_F), scale = max(1, max|w|); the last pencil of a second call carries a NaN in B and
!! must fail alone; the guards between the blocks of w and z must survive both calls.
program gvbatch_caller
  use eigen_libs_mod
  implicit none
  integer, parameter :: nb = 4, gap = 5
  integer :: n(nb), lda(nb), ldb(nb), ldz(nb), info(nb), i, j, k, m, pass
  integer(8) :: ia(nb), ib(nb), iw(nb), iz(nb), ta, tb, tw, tz, p
  real(8), allocatable :: a(:), b(:), z(:), w(:)
  real(8), allocatable :: am(:, :), bm(:, :), h(:, :), zm(:, :), um(:, :), r(:, :), s(:), wk(:)
  logical, allocatable :: wmine(:)
  real(8) :: gres, gorth, gfac, nan, scale
  real(8), parameter :: guard = -7.25d0
  n = (/7, 30, 70, 12/)
  lda = n + 3
  ldb = n + 2
  ldz = n + 1
  ta = 1; tb = 1; tw = 1; tz = 1
  do k = 1, nb
    ia(k) = ta + gap; ta = ia(k) + int(lda(k), 8) * n(k)
    ib(k) = tb + gap; tb = ib(k) + int(ldb(k), 8) * n(k)
    iw(k) = tw + gap; tw = iw(k) + n(k)
    iz(k) = tz + gap; tz = iz(k) + int(ldz(k), 8) * n(k)
  end do
  allocate(a(ta + gap), b(tb + gap), w(tw + gap), z(tz + gap), wmine(tw + gap))
  call eigen_init()
  nan = 0d0
  nan = nan / nan
  gres = 0d0
  gorth = 0d0
  gfac = 0d0
  do pass = 1, 2
    a = nan
    b = nan
    do k = 1, nb
      m = n(k)
      call overlap(k, m)
      do j = 1, m
        do i = 1, j
          a(ia(k) + (i - 1) + int(lda(k), 8) * (j - 1)) = dble(k) * dble(min(i, j))
          b(ib(k) + (i - 1) + int(ldb(k), 8) * (j - 1)) = bm(i, j)
        end do
      end do
    end do
    info = 77
    w = guard
    z = guard
    if (pass == 1) then
      call eigen_gev_vbatch(nb, n, a, ia, lda, b, ib, ldb, w, iw, z, iz, ldz)
    else
      b(ib(nb) + 2 + int(ldb(nb), 8) * 6) = nan
      call eigen_gev_vbatch(nb, n, a, ia, lda, b, ib, ldb, w, iw, z, iz, ldz, mode='N', info=info)
      if (any(info(1:nb - 1) /= 0) .or. info(nb) /= -5 .or. w(iw(nb)) == w(iw(nb))) then
        print *, "eigen_gev_vbatch: wrong per-block status", info
        stop 1
      end if
      if (any(z /= guard)) then
        print *, "eigen_gev_vbatch: mode N wrote z"
        stop 1
      end if
    end if
    wmine = .false.
    do k = 1, nb
      wmine(iw(k) : iw(k) + n(k) - 1) = .true.
    end do
    if (any(.not. wmine .and. w /= guard)) then
      print *, "eigen_gev_vbatch: w was written between the blocks"
      stop 1
    end if
    do k = 1, merge(nb, nb - 1, pass == 1)
      m = n(k)
      call overlap(k, m)
      allocate(am(m, m), zm(m, m), um(m, m), r(m, m), wk(m))
      do j = 1, m
        do i = 1, m
          am(i, j) = dble(k) * dble(min(i, j))
        end do
      end do
      wk = w(iw(k) : iw(k) + m - 1)
      if (any(wk(2:m) < wk(1:m - 1))) then
        print *, "eigen_gev_vbatch: eigenvalues not ascending, block", k
        stop 1
      end if
      scale = max(1d0, maxval(abs(wk)))
      um = 0d0
      do j = 1, m
        p = ib(k) + int(ldb(k), 8) * (j - 1)
        um(1:j, j) = b(p : p + j - 1)
        if (b(p + m) == b(p + m)) then
          print *, "eigen_gev_vbatch: a padding row of b was written", k, j
          stop 1
        end if
      end do
      r = matmul(transpose(um), um) - bm
      gfac = max(gfac, sqrt(sum(r * r)) / (1d-12 * m * sqrt(sum(bm**2))))
      if (pass == 1) then
        do j = 1, m
          p = iz(k) + int(ldz(k), 8) * (j - 1)
          zm(:, j) = z(p : p + m - 1)
          if (z(p + m) /= guard) then
            print *, "eigen_gev_vbatch: a padding row of z was written", k, j
            stop 1
          end if
        end do
        r = matmul(bm, zm)
        do j = 1, m
          r(:, j) = r(:, j) * wk(j)
        end do
        r = matmul(am, zm) - r
        gres = max(gres, sqrt(sum(r * r)) / (1d-12 * scale * m))
        r = matmul(transpose(zm), matmul(bm, zm))
        do j = 1, m
          r(j, j) = r(j, j) - 1d0
        end do
        gorth = max(gorth, sqrt(sum(r * r)) / (1d-12 * m))
      end if
      deallocate(am, zm, um, r, wk)
    end do
  end do
  print *, "eigen_gev_vbatch residual in units of its gate =", gres
  print *, "eigen_gev_vbatch B-orthogonality in units of its gate =", gorth
  print *, "eigen_gev_vbatch factor in units of its gate =", gfac
  call eigen_free()
contains
  !> bm(m, m) = H^T diag(s) H, H the Helmert matrix of order m, s(i) = k + i / m
  subroutine overlap(k, m)
    integer, intent(in) :: k, m
    integer :: i, j
    if (allocated(bm)) deallocate(bm, h, s)
    allocate(bm(m, m), h(m, m), s(m))
    h = 0d0
    h(1, :) = 1d0 / sqrt(dble(m))
    do i = 2, m
      h(i, 1:i - 1) = 1d0 / sqrt(dble(i) * dble(i - 1))
      h(i, i) = -dble(i - 1) / sqrt(dble(i) * dble(i - 1))
    end do
    do i = 1, m
      s(i) = dble(k) + dble(i) / dble(m)
    end do
    do j = 1, m
      do i = 1, m
        bm(i, j) = sum(h(:, i) * s * h(:, j))
      end do
    end do
  end subroutine overlap
end program gvbatch_caller
