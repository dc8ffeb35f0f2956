!> Fortran caller of eigen_gev_batch_range (an extension: the reference solves one pencil per call, completely) on four pencils:
!! A = the Frank matrix (benchmark/mat_set.f:638-647) scaled by 1 .. 4, B = H^T diag(s) H with H the Helmert matrix and
!! s(i) = k + i / n.  The first call asks for the six largest eigenpairs, the second for the three smallest eigenvalues beside a
!! pencil with a NaN in B, which must fail alone.  Prints, worst over the pencils and in units of the gate, ||A Z - B Z W||_F /
!! (1e-12 scale n), ||Z^T B Z - I_m||_F / (1e-12 n) and ||U^T U - B||_F / (1e-12 n ||B||_F), scale = max(1, max|w|).
program gbatch_range_caller
  use eigen_libs_mod
  implicit none
  integer, parameter :: n = 30, nb = 4, lda = n + 1, ldb = n + 3, ldz = n + 2, mw = 6
  real(8), allocatable :: a(:, :, :), b(:, :, :), z(:, :, :), w(:, :)
  real(8) :: am(n, n), bm(n, n, nb), h(n, n), zm(n, mw), um(n, n), r(n, n), rz(n, mw), rm(mw, mw), s(n)
  integer :: info(nb), i, j, k, pass, il, iu, m
  real(8) :: gres, gorth, gfac, nan, scale
  allocate(a(lda, n, nb), b(ldb, n, nb), z(ldz, mw, nb), w(mw, nb))
  call eigen_init()
  nan = 0d0
  nan = nan / nan
  h = 0d0
  h(1, :) = 1d0 / sqrt(dble(n))
  do i = 2, n
    h(i, 1:i - 1) = 1d0 / sqrt(dble(i) * dble(i - 1))
    h(i, i) = -dble(i - 1) / sqrt(dble(i) * dble(i - 1))
  end do
  do k = 1, nb
    do i = 1, n
      s(i) = dble(k) + dble(i) / dble(n)
    end do
    do j = 1, n
      do i = 1, n
        bm(i, j, k) = sum(h(:, i) * s * h(:, j))
      end do
    end do
  end do
  gres = 0d0
  gorth = 0d0
  gfac = 0d0
  do pass = 1, 2
    a = nan
    b = nan
    do k = 1, nb
      do j = 1, n
        do i = 1, j
          a(i, j, k) = dble(k) * dble(min(i, j))
          b(i, j, k) = bm(i, j, k)
        end do
      end do
    end do
    info = 77
    w = nan
    if (pass == 1) then
      il = n - mw + 1
      iu = n
      call eigen_gev_batch_range(n, nb, il, iu, a, lda, b, ldb, w, z, ldz)
    else
      il = 1
      iu = 3
      b(3, 7, nb) = nan
      call eigen_gev_batch_range(n, nb, il, iu, a, lda, b, ldb, w, z, ldz, mode='N', info=info)
      if (any(info(1:nb - 1) /= 0) .or. info(nb) /= -5 .or. w(1, nb) == w(1, nb)) then
        print *, "eigen_gev_batch_range: wrong per-pencil status", info
        stop 1
      end if
    end if
    m = iu - il + 1
    do k = 1, merge(nb, nb - 1, pass == 1)
      do j = 1, n
        do i = 1, n
          am(i, j) = dble(k) * dble(min(i, j))
        end do
      end do
      if (any(w(2:m, k) < w(1:m - 1, k))) then
        print *, "eigen_gev_batch_range: eigenvalues not ascending, pencil", k
        stop 1
      end if
      scale = max(1d0, maxval(abs(w(1:m, k))))
      um = 0d0
      do j = 1, n
        um(1:j, j) = b(1:j, j, k)
      end do
      r = matmul(transpose(um), um) - bm(:, :, k)
      gfac = max(gfac, sqrt(sum(r * r)) / (1d-12 * n * sqrt(sum(bm(:, :, k)**2))))
      if (pass == 1) then
        zm = z(1:n, 1:m, k)
        rz = matmul(bm(:, :, k), zm)
        do j = 1, m
          rz(:, j) = rz(:, j) * w(j, k)
        end do
        rz = matmul(am, zm) - rz
        gres = max(gres, sqrt(sum(rz * rz)) / (1d-12 * scale * n))
        rm = matmul(transpose(zm), matmul(bm(:, :, k), zm))
        do j = 1, m
          rm(j, j) = rm(j, j) - 1d0
        end do
        gorth = max(gorth, sqrt(sum(rm * rm)) / (1d-12 * n))
      end if
    end do
  end do
  print *, "eigen_gev_batch_range N=", n, " residual in units of its gate =", gres
  print *, "eigen_gev_batch_range N=", n, " B-orthogonality in units of its gate =", gorth
  print *, "eigen_gev_batch_range N=", n, " factor in units of its gate =", gfac
  call eigen_free()
end program gbatch_range_caller
