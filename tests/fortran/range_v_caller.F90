!> Fortran caller of eigen_sx_range_v (module eigen_libs_mod) and the external KMATH_EIGEN_GEV_RANGE_V (extensions: the
!! reference has no value-window interface) on the Frank matrix (benchmark/mat_set.f:638-647), n = 200, whose eigenvalues
!! are known in closed form.  argv: vl vu, mid-gap points of that spectrum.  The generalised problem is the pencil of
!! gev_range_caller.F90: A = G K G, B = G G with K = Frank and G = D^1/2, so its spectrum is Frank's as well.
!! Prints m, il and the largest relative eigenvalue error of each call, then an overflow call (mmax = m - 1).
program range_v_caller
  use eigen_libs_mod
  implicit none
  interface
    subroutine KMATH_EIGEN_GEV_RANGE_V(n, vl, vu, mmax, m, il, a, lda, b, ldb, w, z, ldz, mode)
      integer, intent(in) :: n, mmax, lda, ldb, ldz
      real(8), intent(in) :: vl, vu
      integer, intent(out) :: m, il
      real(8), intent(inout) :: a(lda, *), b(ldb, *)
      real(8), intent(inout) :: w(*), z(ldz, *)
      character(*), intent(in), optional :: mode
    end subroutine
  end interface
  integer, parameter :: n = 200, mmax = 64
  integer :: i, j, m, il, m2, il2
  real(8), allocatable :: a(:, :), b(:, :), z(:, :), w(:), d(:)
  real(8) :: vl, vu, err, pi
  character(64) :: arg
  logical :: untouched
  call get_command_argument(1, arg); read(arg, *) vl
  call get_command_argument(2, arg); read(arg, *) vu
  allocate(a(n, n), b(n, n), z(n, mmax), w(mmax), d(n))
  pi = 4d0 * atan(1d0)
  call eigen_init()
  ! ---- eigen_sx_range_v
  do j = 1, n
    do i = 1, n
      a(i, j) = dble(min(i, j))
    end do
  end do
  call eigen_sx_range_v(n, vl, vu, mmax, m, il, a, n, w, z, n)
  print *, "eigen_sx_range_v m =", m, " il =", il, " max rel eigenvalue error =", frank_err(m, il)
  ! ---- KMATH_EIGEN_GEV_RANGE_V, upper triangles only
  do i = 1, n
    d(i) = 1d0 + 9d0 * dble(mod(37 * i, n)) / dble(n)
  end do
  a = 0d0
  b = 0d0
  do j = 1, n
    do i = 1, j
      a(i, j) = sqrt(d(i)) * dble(min(i, j)) * sqrt(d(j))
    end do
    b(j, j) = d(j)
  end do
  call KMATH_EIGEN_GEV_RANGE_V(n, vl, vu, mmax, m, il, a, n, b, n, w, z, n, mode='A')
  print *, "KMATH_EIGEN_GEV_RANGE_V m =", m, " il =", il, " max rel eigenvalue error =", frank_err(m, il)
  ! ---- the window does not fit: m and il come back, w and z stay as they were
  do j = 1, n
    do i = 1, n
      a(i, j) = dble(min(i, j))
    end do
  end do
  w = 7d0
  z = 7d0
  call eigen_sx_range_v(n, vl, vu, m - 1, m2, il2, a, n, w, z, n, mode='A')
  untouched = all(w == 7d0) .and. all(z == 7d0)
  print *, "overflow m =", m2, " il =", il2, " untouched = ", untouched
  call eigen_free()
contains
  real(8) function frank_err(m, il)
    integer, intent(in) :: m, il
    integer :: k
    real(8) :: lam
    frank_err = 0d0
    if (m < 1) frank_err = 1d0
    do k = 1, m
      lam = 1d0 / (2d0 * (1d0 - cos((2 * (n - (il + k - 1) + 1) - 1) * pi / (2 * n + 1))))
      frank_err = max(frank_err, abs(w(k) - lam) / lam)
    end do
  end function
end program range_v_caller
