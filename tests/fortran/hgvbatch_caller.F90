!> Fortran caller of eigen_hgev_vbatch (an extension: the reference has no complex generalised solver) on Hermitian-definite
!! pencils of the orders 7, 30, 60 and 12 packed into flat complex arrays with padded columns and gaps: A = D F D^H with F the
!! Frank matrix (benchmark/mat_set.f:638-647) scaled by 1 .. 4 and D unit phases, B = D H^T diag(s) H D^H with H the Helmert
!! matrix of the block's order and s(i) = k + i / n.  The start indices are 1-based and count complex elements.  Prints, worst
!! over the pencils and in units of the gate, ||A Z - B Z W||_F / (1e-12 scale n), ||Z^H B Z - I||_F / (1e-12 n) and
!! ||U^H U - B||_F / (1e-12 n ||B||_F), scale = max(1, max|w|); the last pencil of a second call carries a NaN in B and must
!! fail alone; the guards between the blocks of w and z must survive both calls.
program hgvbatch_caller
  use eigen_libs_mod
  implicit none
  integer, parameter :: nb = 4, gap = 5
  integer :: n(nb), lda(nb), ldb(nb), ldz(nb), info(nb), i, j, k, m, pass
  integer(8) :: ia(nb), ib(nb), iw(nb), iz(nb), ta, tb, tw, tz, p
  complex(8), allocatable :: a(:), b(:), z(:)
  real(8), allocatable :: w(:)
  complex(8), allocatable :: am(:, :), bm(:, :), zm(:, :), um(:, :), r(:, :), ph(:)
  real(8), allocatable :: h(:, :), s(:), wk(:)
  logical, allocatable :: wmine(:)
  real(8) :: gres, gorth, gfac, nan, scale
  real(8), parameter :: guard = -7.25d0
  n = (/7, 30, 60, 12/)
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
    a = cmplx(nan, nan, 8)
    b = cmplx(nan, nan, 8)
    do k = 1, nb
      m = n(k)
      call pencil(k, m)
      do j = 1, m
        do i = 1, j
          a(ia(k) + (i - 1) + int(lda(k), 8) * (j - 1)) = am(i, j)
          b(ib(k) + (i - 1) + int(ldb(k), 8) * (j - 1)) = bm(i, j)
        end do
        ! of the diagonals only the real parts are read
        a(ia(k) + (j - 1) + int(lda(k), 8) * (j - 1)) = cmplx(dble(am(j, j)), nan, 8)
        b(ib(k) + (j - 1) + int(ldb(k), 8) * (j - 1)) = cmplx(dble(bm(j, j)), nan, 8)
      end do
    end do
    info = 77
    w = guard
    z = cmplx(guard, guard, 8)
    if (pass == 1) then
      call eigen_hgev_vbatch(nb, n, a, ia, lda, b, ib, ldb, w, iw, z, iz, ldz)
    else
      b(ib(nb) + 2 + int(ldb(nb), 8) * 6) = cmplx(1d0, nan, 8)
      call eigen_hgev_vbatch(nb, n, a, ia, lda, b, ib, ldb, w, iw, z, iz, ldz, mode='N', info=info)
      if (any(info(1:nb - 1) /= 0) .or. info(nb) /= -5 .or. w(iw(nb)) == w(iw(nb))) then
        print *, "eigen_hgev_vbatch: wrong per-block status", info
        stop 1
      end if
      if (any(z /= cmplx(guard, guard, 8))) then
        print *, "eigen_hgev_vbatch: mode N wrote z"
        stop 1
      end if
    end if
    wmine = .false.
    do k = 1, nb
      wmine(iw(k) : iw(k) + n(k) - 1) = .true.
    end do
    if (any(.not. wmine .and. w /= guard)) then
      print *, "eigen_hgev_vbatch: w was written between the blocks"
      stop 1
    end if
    do k = 1, merge(nb, nb - 1, pass == 1)
      m = n(k)
      call pencil(k, m)
      allocate(zm(m, m), um(m, m), r(m, m), wk(m))
      wk = w(iw(k) : iw(k) + m - 1)
      if (any(wk(2:m) < wk(1:m - 1))) then
        print *, "eigen_hgev_vbatch: eigenvalues not ascending, block", k
        stop 1
      end if
      scale = max(1d0, maxval(abs(wk)))
      um = (0d0, 0d0)
      do j = 1, m
        p = ib(k) + int(ldb(k), 8) * (j - 1)
        um(1:j, j) = b(p : p + j - 1)
        if (aimag(um(j, j)) /= 0d0 .or. dble(um(j, j)) <= 0d0) then
          print *, "eigen_hgev_vbatch: the diagonal of U is not real and positive", k, j
          stop 1
        end if
        if (dble(b(p + m)) == dble(b(p + m))) then
          print *, "eigen_hgev_vbatch: a padding row of b was written", k, j
          stop 1
        end if
      end do
      r = matmul(conjg(transpose(um)), um) - bm
      gfac = max(gfac, sqrt(sum(abs(r)**2)) / (1d-12 * m * sqrt(sum(abs(bm)**2))))
      if (pass == 1) then
        do j = 1, m
          p = iz(k) + int(ldz(k), 8) * (j - 1)
          zm(:, j) = z(p : p + m - 1)
          if (z(p + m) /= cmplx(guard, guard, 8)) then
            print *, "eigen_hgev_vbatch: a padding row of z was written", k, j
            stop 1
          end if
        end do
        r = matmul(bm, zm)
        do j = 1, m
          r(:, j) = r(:, j) * wk(j)
        end do
        r = matmul(am, zm) - r
        gres = max(gres, sqrt(sum(abs(r)**2)) / (1d-12 * scale * m))
        r = matmul(conjg(transpose(zm)), matmul(bm, zm))
        do j = 1, m
          r(j, j) = r(j, j) - 1d0
        end do
        gorth = max(gorth, sqrt(sum(abs(r)**2)) / (1d-12 * m))
      end if
      deallocate(zm, um, r, wk)
    end do
  end do
  print *, "eigen_hgev_vbatch residual in units of its gate =", gres
  print *, "eigen_hgev_vbatch B-orthogonality in units of its gate =", gorth
  print *, "eigen_hgev_vbatch factor in units of its gate =", gfac
  call eigen_free()
contains
  !> am(m, m) = k D F D^H and bm(m, m) = D H^T diag(s) H D^H: F the Frank matrix, H the Helmert matrix of order m,
  !> s(i) = k + i / m, D = diag(exp(0.3 i sqrt(-1)))
  subroutine pencil(k, m)
    integer, intent(in) :: k, m
    integer :: i, j
    if (allocated(bm)) deallocate(am, bm, h, s, ph)
    allocate(am(m, m), bm(m, m), h(m, m), s(m), ph(m))
    h = 0d0
    h(1, :) = 1d0 / sqrt(dble(m))
    do i = 2, m
      h(i, 1:i - 1) = 1d0 / sqrt(dble(i) * dble(i - 1))
      h(i, i) = -dble(i - 1) / sqrt(dble(i) * dble(i - 1))
    end do
    do i = 1, m
      s(i) = dble(k) + dble(i) / dble(m)
      ph(i) = cmplx(cos(0.3d0 * i), sin(0.3d0 * i), 8)
    end do
    do j = 1, m
      do i = 1, m
        am(i, j) = dble(k) * dble(min(i, j)) * ph(i) * conjg(ph(j))
        bm(i, j) = sum(h(:, i) * s * h(:, j)) * ph(i) * conjg(ph(j))
      end do
    end do
  end subroutine pencil
end program hgvbatch_caller
