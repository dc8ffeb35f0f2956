!> Fortran caller of eigen_h_batch_range (an extension: the reference solves one matrix per call) on four copies of the phased
!! Frank matrix D F D^H, D = diag(exp(i theta_j)), F the Frank matrix (benchmark/mat_set.f:638-647), scaled by 1, 2, 3 and 4,
!! whose eigenvalues are Frank's, known in closed form: the six largest eigenpairs of each (il = n - 5, iu = n), then the three
!! smallest eigenvalues in mode 'N' with a NaN in the last matrix, which must fail alone.  Prints the worst relative eigenvalue
!! error and the worst residual ||A z - w z|| / (||A|| n eps).
program hbatch_range_caller
  use eigen_libs_mod
  implicit none
  integer, parameter :: n = 30, nb = 4, lda = n + 1, ldz = n + 2, m = 6
  complex(8), allocatable :: a(:, :, :), z(:, :, :), r(:)
  real(8), allocatable :: w(:, :)
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
    a = cmplx(nan, nan, kind=8)
    do k = 1, nb
      do j = 1, n
        do i = 1, j
          a(i, j, k) = aij(i, j, k)
        end do
        a(j, j, k) = cmplx(dble(k) * dble(j), nan, kind=8)   ! of the diagonal the real part only is read
      end do
    end do
    info = 77
    if (pass == 1) then
      il = n - m + 1
      iu = n
      call eigen_h_batch_range(n, nb, il, iu, a, lda, w, z, ldz)
    else
      il = 1
      iu = 3
      a(3, 7, nb) = cmplx(1d0, nan, kind=8)
      call eigen_h_batch_range(n, nb, il, iu, a, lda, w, z, ldz, mode='N', info=info)
      if (any(info(1:nb - 1) /= 0) .or. info(nb) /= -5 .or. w(1, nb) == w(1, nb)) then
        print *, "eigen_h_batch_range: wrong per-matrix status", info
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
              r(i) = r(i) + aij(i, c, k) * z(c, j, k)
            end do
          end do
          res = max(res, sqrt(sum(abs(r)**2)) / (anorm * n * epsilon(1d0)))
        end do
      end do
    end if
  end do
  print *, "eigen_h_batch_range N=", n, " max rel eigenvalue error =", err
  print *, "eigen_h_batch_range N=", n, " max residual in n eps ||A|| =", res
  call eigen_free()
contains
  !> element (i, j) of matrix k: d_i conj(d_j) k min(i, j), d_j = exp(i (0.7 j^2 + k))
  complex(8) function aij(i, j, k)
    integer, intent(in) :: i, j, k
    complex(8) :: di, dj
    di = cmplx(cos(0.7d0 * i * i + k), sin(0.7d0 * i * i + k), kind=8)
    dj = cmplx(cos(0.7d0 * j * j + k), sin(0.7d0 * j * j + k), kind=8)
    aij = di * conjg(dj) * dble(k) * dble(min(i, j))
  end function aij
end program hbatch_range_caller
