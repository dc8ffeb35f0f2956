!> Fortran caller of KMATH_EIGEN_GEV_RANGE (an extension: the reference has no Cholesky-route or index-range generalised
!! solver) on a known answer: A = G K G, B = G G with K the Frank matrix (benchmark/mat_set.f:638-647) and G = D^1/2
!! (D positive diagonal), so A x = lambda B x turns into K y = lambda y (y = G x) and the spectrum is Frank's.
!! Window [3, 40] of n = 200; prints the eigenvalue error and the two gates of benchmark/KMATH_EIGEN_GEV_check.f.
program gev_range_caller
  use eigen_libs_mod
  implicit none
  interface
    subroutine KMATH_EIGEN_GEV_RANGE(n, il, iu, a, lda, b, ldb, w, z, ldz, mode)
      integer, intent(in) :: n, il, iu, lda, ldb, ldz
      real(8), intent(inout) :: a(lda, *), b(ldb, *)
      real(8), intent(inout) :: w(*), z(ldz, *)
      character(*), intent(in), optional :: mode
    end subroutine
  end interface
  integer :: n, il, iu, m, i, j
  real(8), allocatable :: a(:, :), b(:, :), z(:, :), w(:), wn(:), d(:), a0(:, :), b0(:, :), r(:, :), g(:, :)
  real(8) :: lam, err, pi, res, orth, wdiff
  n = 200; il = 3; iu = 40
  m = iu - il + 1
  allocate(a(n, n), b(n, n), z(n, m), w(m), wn(m), d(n), a0(n, n), b0(n, n), r(n, m), g(m, m))
  call eigen_init()
  do i = 1, n
    d(i) = 1d0 + 9d0 * dble(mod(37 * i, n)) / dble(n)
  end do
  a0 = 0d0
  b0 = 0d0
  do j = 1, n
    do i = 1, n
      a0(i, j) = sqrt(d(i)) * dble(min(i, j)) * sqrt(d(j))
    end do
    b0(j, j) = d(j)
  end do
  ! only the upper triangles are passed
  a = 0d0
  b = 0d0
  do j = 1, n
    a(1:j, j) = a0(1:j, j)
    b(j, j) = b0(j, j)
  end do
  call KMATH_EIGEN_GEV_RANGE(n, il, iu, a, n, b, n, w, z, n)
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
  res = sqrt(sum(r * r))
  g = matmul(transpose(z), matmul(b0, z))
  do j = 1, m
    g(j, j) = g(j, j) - 1d0
  end do
  orth = sqrt(sum(g * g))
  ! eigenvalues only, mode given: the same window
  do j = 1, n
    a(:, j) = 0d0
    a(1:j, j) = a0(1:j, j)
    b(:, j) = 0d0
    b(j, j) = b0(j, j)
  end do
  call KMATH_EIGEN_GEV_RANGE(n, il, iu, a, n, b, n, wn, z, n, mode='N')
  wdiff = maxval(abs(wn - w))
  print *, "KMATH_EIGEN_GEV_RANGE N=", n, " max rel eigenvalue error =", err
  print *, "max |w| =", maxval(abs(w))
  print *, "residual norm =", res
  print *, "B-orthogonality norm =", orth
  print *, "mode N difference =", wdiff
  call eigen_free()
end program gev_range_caller
