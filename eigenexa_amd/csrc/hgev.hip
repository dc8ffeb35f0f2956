// hgev.hip -- KMATH_EIGEN_HGEV: the complex Hermitian-definite generalised problem A x = lambda B x.
//
// EXTENSION: the reference has no complex generalised solver.  This one follows the reference's method for the real case
// (KMATH_EIGEN_GEV_1, src/KMATH_EIGEN_GEV_1.F:57-139: two eigensolves and three products) over complex numbers, with the
// same argument list and on-exit contract as KMATH_EIGEN_GEV (gev.hip gev_dev / gev_dev_mg):
//   eigen_h(B, 'X'):  B = U diag(mu) U^H          (mu_min <= 0: "Matrix B is not positive definite!", EIGX_ERR_NOT_SPD)
//   F = U diag(mu)^-1/2 ;  C = F^H (A F) ;  eigen_h(C, 'X'):  C = Y diag(w) Y^H ;  Z = F Y       (Z^H B Z = I)
// On exit a holds Y, b holds F, w is ascending, z = F Y; timers [0..4] = total, eigen_h(B), forming C, eigen_h(C), Z = F Y.
// Inputs as for eigen_h: interleaved complex(8), leading dimensions in complex elements, only the upper triangles of a and
// b are read, Im of their diagonals is ignored; a non-finite significant entry of a or b returns EIGX_ERR_NONFINITE with
// w = NaN (a is scanned before B's solve).  A is never scaled here, so eigen_h's overflow above a matrix scale of about
// 1e77 is inherited.
//
// The three complex products are real fp64 MFMA GEMMs (dgemm_dev) on split planes, as in herm.hip; the planes, their
// conversions from and to the interleaved arrays and the one-GPU product are those of zplanes.hip:
//   one GPU: four real products per complex product with beta accumulation (zgemm_planes: Tr = Ar Fr - Ai Fi, Ti = Ar Fi + Ai Fr).
//            Stacking K to 2n instead would need two more n^2 planes for the same flops; the extra pass over C that
//            the four-product form costs is ~1 ms at N = 8192 against ~45 ms of MFMA work per complex product.
//            C = F^H T computes only the tiles that meet the upper triangle (tri_mode 1): eigen_h reads nothing else.
//   several ranks: the 2-D cyclic blocks, nothing gathered.  A's lower triangle and F^H come from dist_transpose of each
//            plane; a complex SUMMA gathers both planes of a panel in one message and runs two products with K = 2 kb
//            ([Xr | Xi] times stacked panels of B; the conjugation of F^H is folded into the stacked panels' signs);
//            C's product runs tri_mode 2.  Workspace: 8 planes of n^2/P (A, the transposes / C, F, T), the transposes'
//            exchange buffers (~2 n^2/P) and the panels: within 12 n^2/P doubles + 1 MiB.
#include "eigx_context.h"
#include "eigx_comm.h"
#include "../../include/eigenexa_amd.h"
#include <algorithm>
#include <string>

namespace eigx {

namespace {

// several ranks: below the global diagonal A := conj(A^T), from the transposed planes (Xr, Xi) = (Ar^T, Ai^T)
__global__ void hg_merge_kernel(double* __restrict__ Ar, double* __restrict__ Ai, const double* __restrict__ Xr,
                                const double* __restrict__ Xi, int ld, int nr, int nc, int Px, int px, int Py, int py) {
  for (int lc = blockIdx.y; lc < nc; lc += gridDim.y) {
    const int gc = lc * Py + py;
    for (int lr = blockIdx.x * blockDim.x + threadIdx.x; lr < nr; lr += gridDim.x * blockDim.x) {
      if (lr * Px + px <= gc) continue;
      const size_t o = (size_t)lr + (size_t)lc * ld;
      Ar[o] = Xr[o];
      Ai[o] = -Xi[o];
    }
  }
}

// complex SUMMA, B side: gathered rows of both planes recv[q'][pl][j][rr] (global k = k0 + rr Px + q') -> the two stacked
// panels, rows in the order of the gathered A columns (pos = q 2 kbl_y + pl kbl_y + c for k - k0 = c Py + q, plane pl).
// With X = Xr + i sa Xi on the A side:  Re(X B) = [Xr | Xi] B1,  B1 = [Br; -sa Bi];  Im(X B) = [Xr | Xi] B2,  B2 = [Bi; sa Br]
__global__ void hg_unpack_b_kernel(const double* __restrict__ recv, int Px, int Py, int kbl_x, int kbl_y, int ncp, int kb,
                                   double sa, double* __restrict__ B1, double* __restrict__ B2) {
  const int j = blockIdx.y, q = blockIdx.z;
  for (int rr = blockIdx.x * blockDim.x + threadIdx.x; rr < kbl_x; rr += gridDim.x * blockDim.x) {
    const int dk = rr * Px + q;
    const size_t pos = (size_t)j * 2 * kb + (size_t)(dk % Py) * 2 * kbl_y + dk / Py;
    const double br = recv[(((size_t)q * 2) * ncp + j) * kbl_x + rr];
    const double bi = recv[(((size_t)q * 2 + 1) * ncp + j) * kbl_x + rr];
    B1[pos] = br; B1[pos + kbl_y] = -sa * bi;
    B2[pos] = bi; B2[pos + kbl_y] = sa * br;
  }
}

// C = X B on the 2-D cyclic blocks (all n x n, complete matrices), complex on split planes, X = Xr + i sa Xi (sa = -1:
// the conjugate of the stored planes).  tri: only the tiles of C that meet the upper triangle (tri_mode 2).  Synchronous.
int zsumma(Context& ctx, int n, const ZPlanes& X, int ldx, double sa, const ZPlanes& B, int ldb, const ZPlanes& C, int ldc,
           bool tri) {
  const Grid& G = ctx.grid;
  hipStream_t st = ctx.stream;
  const int nr = local_count(n, G.Px, G.px), nc = local_count(n, G.Py, G.py);
  // panel width about n / 16 between 64 and 512: both planes travel, and the panels stay within ~2 n^2/P + 1 MiB
  const int kb_want = (n < 64) ? n : (n / 16 < 64 ? 64 : (n / 16 > 512 ? 512 : n / 16));
  const SummaPlan p = summa_plan(G, n, kb_want);
  const int kb = p.kb, kbl_x = p.kbl_x, kbl_y = p.kbl_y, nrp = p.nrp, ncp = p.ncp;
  double* sendA = ctx.pool.get_t<double>("hgev.sa", (size_t)2 * nrp * kbl_y);
  double* Ap = ctx.pool.get_t<double>("hgev.pa", (size_t)2 * nrp * kb);
  double* sendB = ctx.pool.get_t<double>("hgev.sb", (size_t)2 * kbl_x * ncp);
  double* recvB = ctx.pool.get_t<double>("hgev.rb", (size_t)2 * kb * ncp);
  double* B1 = ctx.pool.get_t<double>("hgev.pb", (size_t)4 * kb * ncp);
  double* B2 = B1 + (size_t)2 * kb * ncp;
  for (int k0 = 0; k0 < n; k0 += kb) {
    summa_pack_a(st, p, X.r, ldx, nr, nc, k0 / G.Py, sendA);
    summa_pack_a(st, p, X.i, ldx, nr, nc, k0 / G.Py, sendA + (size_t)nrp * kbl_y);
    comm_allgather(ctx, COMM_Y, sendA, Ap, (size_t)2 * nrp * kbl_y, st);     // Ap(:, q 2kbl_y + pl kbl_y + c)
    summa_pack_b(st, p, B.r, ldb, nr, nc, k0 / G.Px, sendB);
    summa_pack_b(st, p, B.i, ldb, nr, nc, k0 / G.Px, sendB + (size_t)kbl_x * ncp);
    comm_allgather(ctx, COMM_X, sendB, recvB, (size_t)2 * kbl_x * ncp, st);
    hipLaunchKernelGGL(hg_unpack_b_kernel, dim3(ceil_div(kbl_x, 256), ncp, G.Px), dim3(256), 0, st, (const double*)recvB, G.Px,
                       G.Py, kbl_x, kbl_y, ncp, kb, sa, B1, B2);
    const double beta = k0 == 0 ? 0.0 : 1.0;
    if (nr > 0 && nc > 0) {
      dgemm_dev(st, 'N', 'N', nr, nc, 2 * kb, 1.0, Ap, nrp, B1, 2 * kb, beta, C.r, ldc, tri ? 2 : 0, tri ? &G : nullptr);
      dgemm_dev(st, 'N', 'N', nr, nc, 2 * kb, 1.0, Ap, nrp, B2, 2 * kb, beta, C.i, ldc, tri ? 2 : 0, tri ? &G : nullptr);
    }
  }
  EIGX_HIP_CHECK(hipStreamSynchronize(st));
  return comm_failed(ctx) ? EIGX_ERR_INTERNAL : EIGX_OK;
}

// eigen_h's default panel widths (eigen_NB_f, eigen_NB_b)
constexpr int HG_MF = 48, HG_MB = 128;

// Several ranks: the 2-D cyclic blocks, nothing gathered
int hgev_dev_mg(Context& ctx, int n, double* a, int lda, double* b, int ldb, double* w, double* z, int ldz) {
  const Grid G = ctx.grid;
  const int nr = local_count(n, G.Px, G.px), nc = local_count(n, G.Py, G.py);
  const int lmin = nr > 1 ? nr : 1;
  GevFrame Fr(ctx);
  if (const int rc0 = Fr.begin(n > 0 && a && b && w && z && lda >= lmin && ldb >= lmin && ldz >= lmin)) return rc0;
  hipStream_t st = ctx.stream;
  int rc = eigen_scaling(ctx, a, lda, true, n, w, nullptr);   // NaN / Inf in A: eigen_h's status, before B's solve
  if (rc != EIGX_OK) return rc;
  const int ldt = ((nr > 2 ? nr : 2) + 1) & ~1;
  const size_t pl = (size_t)ldt * (nc > 0 ? nc : 1);
  double* planes = ctx.pool.get_t<double>("hgev.planes", 8 * pl);
  const ZPlanes A = {planes, planes + pl};
  const ZPlanes X = A.at(2 * pl);   // A^T, later C
  const ZPlanes F = A.at(4 * pl);
  const ZPlanes T = A.at(6 * pl);   // A F, later Z
  zsplit(st, a, lda, nr, nc, true, A, ldt, nullptr, G);
  dist_transpose(ctx, n, A.r, ldt, X.r, ldt, st, "hgev");
  dist_transpose(ctx, n, A.i, ldt, X.i, ldt, st, "hgev");
  if (nr > 0 && nc > 0)
    hipLaunchKernelGGL(hg_merge_kernel, zcol_grid(nr, nc), dim3(256), 0, st, A.r, A.i, X.r, X.i, ldt, nr, nc, G.Px, G.px, G.Py, G.py);
  EIGX_HIP_CHECK(hipStreamSynchronize(st));
  if (comm_failed(ctx)) return EIGX_ERR_INTERNAL;
  rc = herm_solve_dev(ctx, n, n, b, ldb, w, z, ldz, HG_MF, HG_MB, 'X');                   // B = U diag(mu) U^H
  if (rc != EIGX_OK) return rc;
  Fr.mark();
  if (!b_is_positive_definite(ctx, w)) return EIGX_ERR_NOT_SPD;
  zsplit(st, z, ldz, nr, nc, false, F, ldt, w, G);                                          // F = U diag(mu)^-1/2
  zjoin(st, F, ldt, nr, nc, false, b, ldb, G);
  rc = zsumma(ctx, n, A, ldt, 1.0, F, ldt, T, ldt, false);                                  // T = A F
  if (rc != EIGX_OK) return rc;
  dist_transpose(ctx, n, F.r, ldt, A.r, ldt, st, "hgev");                                   // F^T planes (A is done)
  dist_transpose(ctx, n, F.i, ldt, A.i, ldt, st, "hgev");
  rc = zsumma(ctx, n, A, ldt, -1.0, T, ldt, X, ldt, true);                                  // C = F^H T, upper tiles
  if (rc != EIGX_OK) return rc;
  zjoin(st, X, ldt, nr, nc, true, z, ldz, G);
  EIGX_HIP_CHECK(hipStreamSynchronize(st));
  Fr.mark();
  rc = herm_solve_dev(ctx, n, n, z, ldz, w, a, lda, HG_MF, HG_MB, 'X');                   // C = Y diag(w) Y^H, Y in a
  if (rc != EIGX_OK) return rc;
  Fr.mark();
  zsplit(st, a, lda, nr, nc, false, A, ldt, nullptr, G);
  rc = zsumma(ctx, n, F, ldt, 1.0, A, ldt, T, ldt, false);                                  // Z = F Y
  if (rc != EIGX_OK) return rc;
  zjoin(st, T, ldt, nr, nc, false, z, ldz, G);
  EIGX_HIP_CHECK(hipStreamSynchronize(st));
  return Fr.finish();
}

}  // namespace

int hgev_dev(Context& ctx, int n, double* a, int lda, double* b, int ldb, double* w, double* z, int ldz) {
  if (!ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  if (ctx.grid.nranks != 1) return hgev_dev_mg(ctx, n, a, lda, b, ldb, w, z, ldz);
  GevFrame Fr(ctx);
  if (const int rc0 = Fr.begin(n > 0 && a && b && w && z && lda >= n && ldb >= n && ldz >= n)) return rc0;
  hipStream_t st = ctx.stream;
  int rc = eigen_scaling(ctx, a, lda, true, n, w, nullptr);   // NaN / Inf in A: eigen_h's status, before B's solve
  if (rc != EIGX_OK) return rc;
  const int ld = pad_ld(n);
  const size_t pl = (size_t)ld * n;
  const ZPlanes A = {ctx.pool.get_t<double>("hgev.ar", pl), ctx.pool.get_t<double>("hgev.ai", pl)};   // A, later C, later Z
  const ZPlanes F = {ctx.pool.get_t<double>("hgev.fr", pl), ctx.pool.get_t<double>("hgev.fi", pl)};
  const ZPlanes T = {ctx.pool.get_t<double>("hgev.tr", pl), ctx.pool.get_t<double>("hgev.ti", pl)};   // A F, later Y
  zexpand(st, a, lda, n, A, ld);
  rc = herm_solve_dev(ctx, n, n, b, ldb, w, z, ldz, HG_MF, HG_MB, 'X');                   // B = U diag(mu) U^H
  if (rc != EIGX_OK) return rc;
  Fr.mark();
  if (!b_is_positive_definite(ctx, w)) return EIGX_ERR_NOT_SPD;
  zsplit(st, z, ldz, n, n, false, F, ld, w);                                                // F = U diag(mu)^-1/2
  zjoin(st, F, ld, n, n, false, b, ldb);
  zgemm_planes(st, 'N', n, n, n, 1.0, A, ld, F, ld, 0.0, T, ld);                            // T = A F
  zgemm_planes(st, 'C', n, n, n, 1.0, F, ld, T, ld, 0.0, A, ld, 1);                         // C = F^H T, upper tiles
  zjoin(st, A, ld, n, n, true, z, ldz);
  EIGX_HIP_CHECK(hipStreamSynchronize(st));
  Fr.mark();
  rc = herm_solve_dev(ctx, n, n, z, ldz, w, a, lda, HG_MF, HG_MB, 'X');                   // C = Y diag(w) Y^H, Y in a
  if (rc != EIGX_OK) return rc;
  Fr.mark();
  zsplit(st, a, lda, n, n, false, T, ld);
  zgemm_planes(st, 'N', n, n, n, 1.0, F, ld, T, ld, 0.0, A, ld);                            // Z = F Y
  zjoin(st, A, ld, n, n, false, z, ldz);
  EIGX_HIP_CHECK(hipStreamSynchronize(st));
  return Fr.finish();
}

int hgev_host(Context& ctx, int n, double* a, int lda, double* b, int ldb, double* w, double* z, int ldz) {
  if (!ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  // host arrays: the rank's 2-D cyclic blocks a(lda, *), b(ldb, *), z(ldz, *), interleaved complex (one rank: the whole matrices)
  const int nr = local_count(n, ctx.grid.Px, ctx.grid.px), nc = local_count(n, ctx.grid.Py, ctx.grid.py);
  if (n <= 0 || !a || !b || !w || !z || lda < nr || ldb < nr || ldz < nr) return EIGX_ERR_BAD_ARG;
  const HostStage S(ctx, 16, nr, nc, a, lda, b, ldb, nc, n);
  const int rc = hgev_dev(ctx, n, S.a, S.ldd, S.b, S.ldd, S.w, S.z, S.ldd);
  S.w_back(w, n);   // in every case (gev_host: on EIGX_OK only): NaN for a non-finite input, as eigen_h
  if (rc != EIGX_OK) return rc;
  S.back(z, ldz, S.z, nc);
  S.back(a, lda, S.a, nc);   // Y
  S.back(b, ldb, S.b, nc);   // F
  return EIGX_OK;
}

// ---- KMATH_EIGEN_HGEV_RANGE[_V]: eigenpairs il .. iu of A x = lambda B x, or those with vl <= lambda < vu, by the Cholesky
// route (EXTENSION, one GPU) ------------------------------------------------------------------------------------------------
// B = U^H U (ztri.hip) -> C = U^-H A U^-1 -> the inner solve of C -> Z = U^-1 Y on the window's columns: the complex
// sibling of gev_range_dev (gev.hip).  4 (1/3 + 5/3 + m/n) n^3 real flops through the MFMA GEMM and ONE eigen_h where
// hgev_dev spends 20 n^3 and two.  B is not scaled (the limitation of gev_range_dev): U carries the square root of B's scale
// and C its inverse; eigen_h scales C itself, but only once it has been formed.
// By index, the inner solve is eigen_h itself with nvec = iu: with il > 1 the columns 1 .. il - 1 of Y are computed and
// dropped, and the workspace holds an n x iu complex Y.  By value, it is herm_range_dev (herm.hip) with the same window on
// C: B is not scaled, so the bounds need no transformation (DESIGN 8e "Generalised"); m is read back and Z = U^-1 Y runs on
// m columns (not at all for m = 0, 'N' and 'C'); Y holds min(mmax, n) columns.  b holds U whenever the call returns EIGX_OK.
// Pool buffers: hgevr.u, hgevr.a, hgevr.cp (two planes of pad_ld(n) x n each), hgevr.c (C interleaved), hgevr.y (mode 'A':
// Y), hgevr.w (n, by index) and the block inverses and panels of ztri.hip.
int hgev_range_dev(Context& ctx, int n, const RangeWindow& W, double* a, int lda, double* b, int ldb, double* w, double* z,
                   int ldz, char mode) {
  if (!ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  if (ctx.grid.nranks != 1) return refuse_several_ranks(ctx);
  mode = upper_case(mode);
  GevFrame Fr(ctx);
  if (const int rc0 = Fr.begin(range_args_ok(n, W, a, lda, w, z, ldz, mode) && b && ldb >= n)) return rc0;
  hipStream_t st = ctx.stream;
  const int wcap = range_w_cap(W, mode);
  // both significant triangles are scanned before anything is factored
  int rc = eigen_scaling(ctx, a, lda, true, n, w, nullptr, wcap);
  if (rc == EIGX_OK) rc = eigen_scaling(ctx, b, ldb, true, n, w, nullptr, wcap);
  if (rc != EIGX_OK) {
    if (W.by_value) *W.m_out = 0;
    return rc;
  }
  const int ld = pad_ld(n);
  const ZPlanes U = zplanes(ctx, "hgevr.u", ld, n);
  const ZPlanes A = zplanes(ctx, "hgevr.a", ld, n);     // A, later the window's columns of Y, later Z
  const ZPlanes Cp = zplanes(ctx, "hgevr.cp", ld, n);
  zsplit(st, b, ldb, n, n, true, U, ld);
  if (zchol_upper_dev(ctx, n, U, ld) != EIGX_OK) return report_not_spd(ctx);
  zjoin(st, U, ld, n, n, true, b, ldb);
  Fr.mark();
  const ZTriInv V = ztri_inverses_dev(ctx, n, U, ld);   // once per factor: the three solves below share them
  zexpand(st, a, lda, n, A, ld);
  hgev_reduce_dev(ctx, n, A, ld, U, ld, V, Cp, ld);
  const int ldc = host_ld(n);
  double* c = ctx.pool.get_t<double>("hgevr.c", (size_t)2 * ldc * n);
  zjoin(st, Cp, ld, n, n, true, c, ldc);
  EIGX_HIP_CHECK(hipStreamSynchronize(st));
  Fr.mark();
  int m = W.m();
  const double* ywin = nullptr;   // the window's columns of Y
  if (W.by_value) {
    double* y = mode == 'A' ? ctx.pool.get_t<double>("hgevr.y", (size_t)2 * ldc * range_z_cap(n, W, mode)) : nullptr;
    rc = herm_range_dev(ctx, n, W, c, ldc, w, y, ldc, HG_MF, HG_MB, mode);   // the pairs of C with vl <= lambda < vu
    if (rc != EIGX_OK) return rc;
    m = mode == 'C' ? 0 : *W.m_out;
    ywin = y;
  } else {
    const int il = W.il, iu = W.iu;
    double* wn = ctx.pool.get_t<double>("hgevr.w", (size_t)n);
    double* y = mode == 'A' ? ctx.pool.get_t<double>("hgevr.y", (size_t)2 * ldc * iu) : nullptr;
    rc = herm_solve_dev(ctx, n, iu, c, ldc, wn, y, ldc, HG_MF, HG_MB, mode);    // C = Y diag(w) Y^H, the lowest iu
    if (rc == EIGX_OK || rc == EIGX_ERR_NONFINITE)
      EIGX_HIP_CHECK(hipMemcpyAsync(w, wn + (il - 1), (size_t)m * 8, hipMemcpyDeviceToDevice, st));
    EIGX_HIP_CHECK(hipStreamSynchronize(st));
    if (rc != EIGX_OK) return rc;
    ywin = y + (size_t)2 * ldc * (il - 1);
  }
  Fr.mark();
  if (mode == 'A' && m > 0) {
    zsplit(st, ywin, ldc, n, m, false, A, ld);
    ztrsm_upper_dev(ctx, 'N', n, m, U, ld, A, ld, V);   // Z = U^-1 Y
    zjoin(st, A, ld, n, m, false, z, ldz);
    EIGX_HIP_CHECK(hipStreamSynchronize(st));
  }
  return Fr.finish();
}

int hgev_range_host(Context& ctx, int n, const RangeWindow& W, double* a, int lda, double* b, int ldb, double* w, double* z,
                    int ldz, char mode) {
  return range_host_form(
      ctx, n, W, 16, a, lda, true, b, ldb, w, z, ldz, mode,
      [&](const HostStage& S) { return hgev_range_dev(ctx, n, W, S.a, S.ldd, S.b, S.ldd, S.w, S.z, S.ldd, mode); },
      [&](const HostStage& S) { S.back(b, ldb, S.b, n); });   // U in the upper triangle; a is not returned
}

}  // namespace eigx

using namespace eigx;

extern "C" {

int eigx_hgev(int n, double* a, int lda, double* b, int ldb, double* w, double* z, int ldz) {
  return eigx_guard(g_ctx, [&] { return hgev_host(g_ctx, n, a, lda, b, ldb, w, z, ldz); });
}
int eigx_hgev_dev(int n, double* a, int lda, double* b, int ldb, double* w, double* z, int ldz) {
  return eigx_guard(g_ctx, [&] { return hgev_dev(g_ctx, n, a, lda, b, ldb, w, z, ldz); });
}

// EXTENSION: eigenpairs il .. iu of the complex problem by the Cholesky route (one GPU); see hgev_range_dev
int eigx_hgev_range(int n, int il, int iu, double* a, int lda, double* b, int ldb, double* w, double* z, int ldz, char mode) {
  return eigx_guard(g_ctx, [&] { return hgev_range_host(g_ctx, n, RangeWindow::index(il, iu), a, lda, b, ldb, w, z, ldz, mode); });
}
int eigx_hgev_range_dev(int n, int il, int iu, double* a, int lda, double* b, int ldb, double* w, double* z, int ldz, char mode) {
  return eigx_guard(g_ctx, [&] { return hgev_range_dev(g_ctx, n, RangeWindow::index(il, iu), a, lda, b, ldb, w, z, ldz, mode); });
}
// EXTENSION: the eigenpairs with vl <= lambda < vu of the complex problem; m, il: host pointers in both forms
int eigx_hgev_range_v(int n, double vl, double vu, int mmax, int* m, int* il, double* a, int lda, double* b, int ldb, double* w,
                      double* z, int ldz, char mode) {
  return eigx_guard(g_ctx, [&] {
    return hgev_range_host(g_ctx, n, RangeWindow::value(vl, vu, mmax, m, il), a, lda, b, ldb, w, z, ldz, mode);
  });
}
int eigx_hgev_range_v_dev(int n, double vl, double vu, int mmax, int* m, int* il, double* a, int lda, double* b, int ldb,
                          double* w, double* z, int ldz, char mode) {
  return eigx_guard(g_ctx, [&] {
    return hgev_range_dev(g_ctx, n, RangeWindow::value(vl, vu, mmax, m, il), a, lda, b, ldb, w, z, ldz, mode);
  });
}

}  // extern "C"
