!> Fortran caller of eigen_hgev_batch_range (an extension: the reference has no complex generalised solver) on four pencils, those
!! of hgbatch_caller.F90: A = D F D^H with F the Frank matrix (benchmark/mat_set.f:638-647) scaled by 1 .. 4 and
!! D = diag(exp(i theta_j)), theta_j = 0.7 j; B = G G^H / n + 0.1 k I with G(i, j) = cos(i j + k) + i sin(2 i - 3 j + k).  NaN sits
!! in the strict lower triangles, the padding rows and the imaginary parts of both diagonals.  The first call asks for the six
!! largest eigenpairs, the second for the three smallest eigenvalues beside a pencil with a NaN in B, which must fail alone.
!! Prints, worst over the pencils and in units of the gate, ||A Z - B Z W||_F / (1e-12 scale n), ||Z^H B Z - I_m||_F / (1e-12 n)
!! and ||U^H U - B||_F / (1e-12 n ||B||_F), scale = max(1, max|w|).
program hgbatch_range_caller
  use eigen_libs_mod
  implicit none
  integer, parameter :: n = 30, nb = 4, lda = n + 1, ldb = n + 3, ldz = n + 2, mw = 6
  complex(8), allocatable :: a(:, :, :), b(:, :, :), z(:, :, :)
  real(8), allocatable :: w(:, :)
  complex(8) :: am(n, n), bm(n, n, nb), g(n, n), zm(n, mw), um(n, n), r(n, n), rz(n, mw), rm(mw, mw), ph(n)
  integer :: info(nb), i, j, k, pass, il, iu, m
  real(8) :: gres, gorth, gfac, nan, scale
  allocate(a(lda, n, nb), b(ldb, n, nb), z(ldz, mw, nb), w(mw, nb))
  call eigen_init()
  nan = 0d0
  nan = nan / nan
  do j = 1, n
    ph(j) = cmplx(cos(0.7d0 * j), sin(0.7d0 * j), kind=8)
  end do
  do k = 1, nb
    do j = 1, n
      do i = 1, n
        g(i, j) = cmplx(cos(dble(i * j + k)), sin(dble(2 * i - 3 * j + k)), kind=8)
      end do
    end do
    bm(:, :, k) = matmul(g, conjg(transpose(g))) / dble(n)
    do i = 1, n
      bm(i, i, k) = cmplx(dble(bm(i, i, k)) + 0.1d0 * k, 0d0, kind=8)
    end do
  end do
  gres = 0d0
  gorth = 0d0
  gfac = 0d0
  do pass = 1, 2
    a = cmplx(nan, nan, kind=8)
    b = cmplx(nan, nan, kind=8)
    do k = 1, nb
      do j = 1, n
        do i = 1, j
          a(i, j, k) = dble(k) * dble(min(i, j)) * ph(i) * conjg(ph(j))
          b(i, j, k) = bm(i, j, k)
        end do
        a(j, j, k) = cmplx(dble(k) * dble(j), nan, kind=8)
        b(j, j, k) = cmplx(dble(bm(j, j, k)), nan, kind=8)
      end do
    end do
    info = 77
    w = nan
    if (pass == 1) then
      il = n - mw + 1
      iu = n
      call eigen_hgev_batch_range(n, nb, il, iu, a, lda, b, ldb, w, z, ldz)
    else
      il = 1
      iu = 3
      b(3, 7, nb) = cmplx(1d0, nan, kind=8)
      call eigen_hgev_batch_range(n, nb, il, iu, a, lda, b, ldb, w, z, ldz, mode='N', info=info)
      if (any(info(1:nb - 1) /= 0) .or. info(nb) /= -5 .or. w(1, nb) == w(1, nb)) then
        print *, "eigen_hgev_batch_range: wrong per-pencil status", info
        stop 1
      end if
    end if
    m = iu - il + 1
    do k = 1, merge(nb, nb - 1, pass == 1)
      do j = 1, n
        do i = 1, n
          am(i, j) = dble(k) * dble(min(i, j)) * ph(i) * conjg(ph(j))
        end do
      end do
      if (any(w(2:m, k) < w(1:m - 1, k))) then
        print *, "eigen_hgev_batch_range: eigenvalues not ascending, pencil", k
        stop 1
      end if
      scale = max(1d0, maxval(abs(w(1:m, k))))
      um = (0d0, 0d0)
      do j = 1, n
        um(1:j, j) = b(1:j, j, k)
        if (aimag(b(j, j, k)) /= 0d0 .or. .not. dble(b(j, j, k)) > 0d0) then
          print *, "eigen_hgev_batch_range: the diagonal of U is not real and positive, pencil", k
          stop 1
        end if
      end do
      r = matmul(conjg(transpose(um)), um) - bm(:, :, k)
      gfac = max(gfac, sqrt(sum(abs(r)**2)) / (1d-12 * n * sqrt(sum(abs(bm(:, :, k))**2))))
      if (pass == 1) then
        zm = z(1:n, 1:m, k)
        rz = matmul(bm(:, :, k), zm)
        do j = 1, m
          rz(:, j) = rz(:, j) * w(j, k)
        end do
        rz = matmul(am, zm) - rz
        gres = max(gres, sqrt(sum(abs(rz)**2)) / (1d-12 * scale * n))
        rm = matmul(conjg(transpose(zm)), matmul(bm(:, :, k), zm))
        do j = 1, m
          rm(j, j) = rm(j, j) - 1d0
        end do
        gorth = max(gorth, sqrt(sum(abs(rm)**2)) / (1d-12 * n))
      end if
    end do
  end do
  print *, "eigen_hgev_batch_range N=", n, " residual in units of its gate =", gres
  print *, "eigen_hgev_batch_range N=", n, " B-orthogonality in units of its gate =", gorth
  print *, "eigen_hgev_batch_range N=", n, " factor in units of its gate =", gfac
  call eigen_free()
end program hgbatch_range_caller
