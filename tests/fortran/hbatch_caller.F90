!> Fortran caller of eigen_h_batch (an extension: the reference solves one matrix per call) on four copies of the phased
!! Frank matrix D F D^H, D = diag(exp(i theta_j)), F the Frank matrix (benchmark/mat_set.f:638-647), scaled by 1, 2, 3 and
!! 4: the eigenvalues are Frank's, known in closed form; the last matrix of a second call carries a NaN and must fail alone.
program hbatch_caller
  use eigen_libs_mod
  implicit none
  integer, parameter :: n = 30, nb = 4, lda = n + 1, ldz = n + 2
  complex(8), allocatable :: a(:, :, :), z(:, :, :)
  real(8), allocatable :: w(:, :)
  integer :: info(nb), i, j, k, pass
  real(8) :: lam, err, pi, nan
  complex(8) :: di, dj
  allocate(a(lda, n, nb), z(ldz, n, nb), w(n, nb))
  call eigen_init()
  pi = 4d0 * atan(1d0)
  nan = 0d0
  nan = nan / nan
  err = 0d0
  do pass = 1, 2
    a = cmplx(nan, nan, kind=8)
    do k = 1, nb
      do j = 1, n
        dj = cmplx(cos(0.7d0 * j * j + k), sin(0.7d0 * j * j + k), kind=8)
        do i = 1, j
          di = cmplx(cos(0.7d0 * i * i + k), sin(0.7d0 * i * i + k), kind=8)
          a(i, j, k) = di * conjg(dj) * dble(k) * dble(min(i, j))
        end do
        a(j, j, k) = cmplx(dble(k) * dble(j), nan, kind=8)   ! of the diagonal the real part only is read
      end do
    end do
    info = 77
    if (pass == 1) then
      call eigen_h_batch(n, nb, a, lda, w, z, ldz)
    else
      a(3, 7, nb) = cmplx(1d0, nan, kind=8)
      call eigen_h_batch(n, nb, a, lda, w, z, ldz, mode='N', info=info)
      if (any(info(1:nb - 1) /= 0) .or. info(nb) /= -5 .or. w(1, nb) == w(1, nb)) then
        print *, "eigen_h_batch: wrong per-matrix status", info
        stop 1
      end if
    end if
    do k = 1, merge(nb, nb - 1, pass == 1)
      do j = 1, n
        lam = dble(k) / (2d0 * (1d0 - cos((2 * (n - j + 1) - 1) * pi / (2 * n + 1))))
        err = max(err, abs(w(j, k) - lam) / lam)
      end do
    end do
  end do
  print *, "eigen_h_batch N=", n, " max rel eigenvalue error =", err
  call eigen_free()
end program hbatch_caller
