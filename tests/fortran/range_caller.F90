!> Fortran caller of eigen_sx_range / eigen_s_range (an extension: the reference has no index-range interface) on the
!! Frank matrix (benchmark/mat_set.f:638-647), whose eigenvalues are known in closed form: the 40 largest pairs by the
!! pentadiagonal route, then pairs 11 .. 30 by the tridiagonal route.
program range_caller
  use eigen_libs_mod
  implicit none
  integer :: n, i, j, k, il, iu, m, pass
  real(8), allocatable :: a(:, :), z(:, :), w(:)
  real(8) :: lam, err, res, r, s, pi
  n = 300
  allocate(a(n, n), z(n, 40), w(40))
  call eigen_init()
  pi = 4d0 * atan(1d0)
  err = 0d0
  res = 0d0
  do pass = 1, 2
    do j = 1, n
      do i = 1, n
        a(i, j) = dble(min(i, j))
      end do
    end do
    if (pass == 1) then
      il = n - 39; iu = n
      call eigen_sx_range(n, il, iu, a, n, w, z, n)
    else
      il = 11; iu = 30
      call eigen_s_range(n, il, iu, a, n, w, z, n, mode='A')
    end if
    m = iu - il + 1
    do j = 1, m
      lam = 1d0 / (2d0 * (1d0 - cos((2 * (n - (il + j - 1) + 1) - 1) * pi / (2 * n + 1))))
      err = max(err, abs(w(j) - lam) / lam)
      s = 0d0
      do i = 1, n
        r = -w(j) * z(i, j)
        do k = 1, n
          r = r + dble(min(i, k)) * z(k, j)
        end do
        s = s + r * r
      end do
      res = max(res, sqrt(s))
    end do
  end do
  print *, "eigen_range N=", n, " max rel eigenvalue error =", err
  print *, "eigen_range N=", n, " max residual norm =", res
  call eigen_free()
end program range_caller
