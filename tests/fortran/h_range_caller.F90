!> Fortran caller of eigen_h_range / eigen_h_range_v (module eigen_libs_mod) and the external KMATH_EIGEN_HGEV_RANGE_V
!! (extensions: the reference has no range interface) on M = S^H K S, K the Frank matrix (benchmark/mat_set.f:638-647), S unit
!! phases, n = 200: Hermitian with Frank's spectrum, known in closed form.  argv: vl vu, mid-gap points of that spectrum.
!! The generalised problem is the pencil of hgev_range_caller.F90: A = G M G^H, B = G G^H with G = D^1/2.
!! Prints m, il and the largest relative eigenvalue error of each call, then an overflow call (mmax = m - 1).
program h_range_caller
  use eigen_libs_mod
  implicit none
  interface
    subroutine KMATH_EIGEN_HGEV_RANGE_V(n, vl, vu, mmax, m, il, a, lda, b, ldb, w, z, ldz, mode)
      integer, intent(in) :: n, mmax, lda, ldb, ldz
      real(8), intent(in) :: vl, vu
      integer, intent(out) :: m, il
      complex(8), intent(inout) :: a(lda, *), b(ldb, *), z(ldz, *)
      real(8), intent(inout) :: w(*)
      character(*), intent(in), optional :: mode
    end subroutine
  end interface
  integer, parameter :: n = 200, mmax = 64
  integer :: i, j, m, il, m2, il2, mi, ili
  complex(8), allocatable :: a(:, :), b(:, :), z(:, :)
  real(8), allocatable :: w(:), d(:)
  real(8) :: vl, vu, pi
  character(64) :: arg
  logical :: untouched
  call get_command_argument(1, arg); read(arg, *) vl
  call get_command_argument(2, arg); read(arg, *) vu
  allocate(a(n, n), b(n, n), z(n, mmax), w(mmax), d(n))
  pi = 4d0 * atan(1d0)
  do i = 1, n
    d(i) = 1d0 + 9d0 * dble(mod(37 * i, n)) / dble(n)
  end do
  call eigen_init()
  ! ---- eigen_h_range_v, then eigen_h_range on the window it found
  call set_a(.false.)
  call eigen_h_range_v(n, vl, vu, mmax, m, il, a, n, w, z, n)
  print *, "eigen_h_range_v m =", m, " il =", il, " max rel eigenvalue error =", frank_err(m, il)
  mi = m; ili = il
  call set_a(.false.)
  w = 0d0
  if (mi > 0) call eigen_h_range(n, ili, ili + mi - 1, a, n, w, z, n, mode='N')
  print *, "eigen_h_range m =", mi, " il =", ili, " max rel eigenvalue error =", frank_err(mi, ili)
  ! ---- KMATH_EIGEN_HGEV_RANGE_V, upper triangles only
  call set_a(.true.)
  b = (0d0, 0d0)
  do j = 1, n
    b(j, j) = cmplx(d(j), 0d0, kind=8)
  end do
  call KMATH_EIGEN_HGEV_RANGE_V(n, vl, vu, mmax, m, il, a, n, b, n, w, z, n, mode='A')
  print *, "KMATH_EIGEN_HGEV_RANGE_V m =", m, " il =", il, " max rel eigenvalue error =", frank_err(m, il)
  ! ---- the window does not fit: m and il come back, w and z stay as they were
  call set_a(.false.)
  w = 7d0
  z = (7d0, 0d0)
  call eigen_h_range_v(n, vl, vu, mi - 1, m2, il2, a, n, w, z, n, mode='A')
  untouched = all(w == 7d0) .and. all(z == (7d0, 0d0))
  print *, "overflow m =", m2, " il =", il2, " untouched = ", untouched
  call eigen_free()
contains
  ! the upper triangle of S^H K S (scaled: of G S^H K S G)
  subroutine set_a(scaled)
    logical, intent(in) :: scaled
    complex(8) :: si, sj
    a = (0d0, 0d0)
    do j = 1, n
      sj = exp(cmplx(0d0, 0.37d0 * j, kind=8))
      do i = 1, j
        si = exp(cmplx(0d0, 0.37d0 * i, kind=8))
        a(i, j) = conjg(si) * dble(min(i, j)) * sj
        if (scaled) a(i, j) = sqrt(d(i)) * a(i, j) * sqrt(d(j))
      end do
      a(j, j) = cmplx(dble(a(j, j)), 0d0, kind=8)
    end do
  end subroutine
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
end program h_range_caller
