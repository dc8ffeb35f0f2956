!> Fortran caller of KMATH_EIGEN_HGEV_RANGE (an extension: the reference has no complex or Cholesky-route generalised
!! solver) on a known answer: A = G M G^H, B = G G^H with M = S^H K S (K the Frank matrix, benchmark/mat_set.f:638-647,
!! S unit phases) and G = D^1/2 (D positive diagonal), so A x = lambda B x turns into M y = lambda y (y = G^H x) and the
!! spectrum is Frank's.  Window [3, 40] of n = 200; prints the eigenvalues at both ends of the window, the eigenvalue
!! error and the two gates of benchmark/KMATH_EIGEN_GEV_check.f.
program hgev_range_caller
  use eigen_libs_mod
  implicit none
  interface
    subroutine KMATH_EIGEN_HGEV_RANGE(n, il, iu, a, lda, b, ldb, w, z, ldz, mode)
      integer, intent(in) :: n, il, iu, lda, ldb, ldz
      complex(8), intent(inout) :: a(lda, *), b(ldb, *), z(ldz, *)
      real(8), intent(inout) :: w(*)
      character(*), intent(in), optional :: mode
    end subroutine
  end interface
  integer :: n, il, iu, m, i, j
  complex(8), allocatable :: a(:, :), b(:, :), z(:, :), a0(:, :), b0(:, :), r(:, :), g(:, :)
  real(8), allocatable :: w(:), wn(:), d(:)
  complex(8) :: si, sj
  real(8) :: lam, err, pi, res, orth, wdiff
  n = 200; il = 3; iu = 40
  m = iu - il + 1
  allocate(a(n, n), b(n, n), z(n, m), w(m), wn(m), d(n), a0(n, n), b0(n, n), r(n, m), g(m, m))
  call eigen_init()
  do i = 1, n
    d(i) = 1d0 + 9d0 * dble(mod(37 * i, n)) / dble(n)
  end do
  a0 = (0d0, 0d0)
  b0 = (0d0, 0d0)
  do j = 1, n
    sj = exp(cmplx(0d0, 0.37d0 * j, kind=8))
    do i = 1, n
      si = exp(cmplx(0d0, 0.37d0 * i, kind=8))
      a0(i, j) = sqrt(d(i)) * conjg(si) * dble(min(i, j)) * sj * sqrt(d(j))
    end do
    a0(j, j) = cmplx(dble(a0(j, j)), 0d0, kind=8)
    b0(j, j) = cmplx(d(j), 0d0, kind=8)
  end do
  ! only the upper triangles are passed
  a = (0d0, 0d0)
  b = (0d0, 0d0)
  do j = 1, n
    a(1:j, j) = a0(1:j, j)
    b(j, j) = b0(j, j)
  end do
  call KMATH_EIGEN_HGEV_RANGE(n, il, iu, a, n, b, n, w, z, n)
  pi = 4d0 * atan(1d0)
  err = 0d0
  do i = il, iu
    lam = 1d0 / (2d0 * (1d0 - cos((2 * (n - i + 1) - 1) * pi / (2 * n + 1))))
    err = max(err, abs(w(i - il + 1) - lam) / lam)
  end do
  r = matmul(a0, z)
  do j = 1, m
    r(:, j) = r(:, j) - w(j) * matmul(b0, z(:, j))
  end do
  res = sqrt(sum(abs(r)**2))
  g = matmul(conjg(transpose(z)), matmul(b0, z))
  do j = 1, m
    g(j, j) = g(j, j) - 1d0
  end do
  orth = sqrt(sum(abs(g)**2))
  ! eigenvalues only, mode given: the same window
  do j = 1, n
    a(:, j) = (0d0, 0d0)
    a(1:j, j) = a0(1:j, j)
    b(:, j) = (0d0, 0d0)
    b(j, j) = b0(j, j)
  end do
  call KMATH_EIGEN_HGEV_RANGE(n, il, iu, a, n, b, n, wn, z, n, mode='N')
  wdiff = maxval(abs(wn - w))
  print *, "KMATH_EIGEN_HGEV_RANGE N=", n, " max rel eigenvalue error =", err
  print *, "first eigenvalue of the window =", w(1)
  print *, "last eigenvalue of the window =", w(m)
  print *, "max |w| =", maxval(abs(w))
  print *, "residual norm =", res
  print *, "B-orthogonality norm =", orth
  print *, "mode N difference =", wdiff
  call eigen_free()
end program hgev_range_caller
