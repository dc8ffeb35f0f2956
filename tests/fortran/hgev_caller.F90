!> Fortran caller of KMATH_EIGEN_HGEV (an extension: the reference has no complex generalised solver) on a known answer:
!! A = G M G^H, B = G G^H with M = S^H K S (K the Frank matrix, S unit phases) and G = D^1/2 (D positive diagonal), so
!! A x = lambda B x turns into M y = lambda y (y = G^H x) and the spectrum is Frank's (benchmark/mat_set.f:638-647).
program hgev_caller
  use eigen_libs_mod
  implicit none
  integer :: n, i, j
  complex(8), allocatable :: a(:, :), b(:, :), z(:, :)
  real(8), allocatable :: w(:), d(:)
  complex(8) :: si, sj
  real(8) :: lam, err, pi
  n = 200
  allocate(a(n, n), b(n, n), z(n, n), w(n), d(n))
  call eigen_init()
  do i = 1, n
    d(i) = 1d0 + 9d0 * dble(mod(37 * i, n)) / dble(n)
  end do
  a = (0d0, 0d0)
  b = (0d0, 0d0)
  do j = 1, n
    sj = exp(cmplx(0d0, 0.37d0 * j, kind=8))
    do i = 1, j
      si = exp(cmplx(0d0, 0.37d0 * i, kind=8))
      a(i, j) = sqrt(d(i)) * conjg(si) * dble(min(i, j)) * sj * sqrt(d(j))
    end do
    a(j, j) = cmplx(dble(a(j, j)), 0d0, kind=8)
    b(j, j) = cmplx(d(j), 0d0, kind=8)
  end do
  call KMATH_EIGEN_HGEV(n, a, n, b, n, w, z, n)
  pi = 4d0 * atan(1d0)
  err = 0d0
  do i = 1, n
    lam = 1d0 / (2d0 * (1d0 - cos((2 * (n - i + 1) - 1) * pi / (2 * n + 1))))
    err = max(err, abs(w(i) - lam) / lam)
  end do
  print *, "KMATH_EIGEN_HGEV N=", n, " max rel eigenvalue error =", err
  call eigen_free()
end program hgev_caller
