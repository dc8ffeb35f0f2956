!> Fortran caller of eigen_s_batch_range (an extension: the reference solves one matrix per call) on four copies of the Frank
!! matrix (benchmark/mat_set.f:638-647), scaled by 1, 2, 3 and 4, whose eigenvalues are known in closed form: the six largest
!! eigenpairs of each (il = n - 5, iu = n), then the three smallest eigenvalues in mode 'N' with a NaN in the last matrix, which
!! must fail alone.  Prints the worst relative eigenvalue error and the worst residual ||A z - w z|| / (||A|| n eps).
program batch_range_caller
  use eigen_libs_mod
  implicit none
  integer, parameter :: n = 30, nb = 4, lda = n + 1, ldz = n + 2, m = 6
  real(8), allocatable :: a(:, :, :), z(:, :, :), w(:, :), r(:)
  integer :: info(nb), i, j, k, c, pass, il, iu, mm
  real(8) :: lam, err, res, pi, nan, anorm
  allocate(a(lda, n, nb), z(ldz, m, nb), w(m, nb), r(n))
  call eigen_init()
  pi = 4d0 * atan(1d0)
  nan = 0d0
  nan = nan / nan
  err = 0d0
  res = 0d0
  do pass = 1, 2
    a = nan
    do k = 1, nb
      do j = 1, n
        do i = 1, j
          a(i, j, k) = dble(k) * dble(min(i, j))
        end do
      end do
    end do
    info = 77
    if (pass == 1) then
      il = n - m + 1
      iu = n
      call eigen_s_batch_range(n, nb, il, iu, a, lda, w, z, ldz)
    else
      il = 1
      iu = 3
      a(3, 7, nb) = nan
      call eigen_s_batch_range(n, nb, il, iu, a, lda, w, z, ldz, mode='N', info=info)
      if (any(info(1:nb - 1) /= 0) .or. info(nb) /= -5 .or. w(1, nb) == w(1, nb)) then
        print *, "eigen_s_batch_range: wrong per-matrix status", info
        stop 1
      end if
    end if
    mm = iu - il + 1
    do k = 1, merge(nb, nb - 1, pass == 1)
      do j = 1, mm
        lam = dble(k) / (2d0 * (1d0 - cos((2 * (n - (il + j - 1) + 1) - 1) * pi / (2 * n + 1))))
        err = max(err, abs(w(j, k) - lam) / lam)
      end do
    end do
    if (pass == 1) then
      do k = 1, nb
        anorm = 0d0
        do j = 1, n
          do i = 1, n
            anorm = anorm + (dble(k) * dble(min(i, j)))**2
          end do
        end do
        anorm = sqrt(anorm)
        do j = 1, m
          do i = 1, n
            r(i) = -w(j, k) * z(i, j, k)
            do c = 1, n
              r(i) = r(i) + dble(k) * dble(min(i, c)) * z(c, j, k)
            end do
          end do
          res = max(res, sqrt(sum(r**2)) / (anorm * n * epsilon(1d0)))
        end do
      end do
    end if
  end do
  print *, "eigen_s_batch_range N=", n, " max rel eigenvalue error =", err
  print *, "eigen_s_batch_range N=", n, " max residual in n eps ||A|| =", res
  call eigen_free()
end program batch_range_caller
