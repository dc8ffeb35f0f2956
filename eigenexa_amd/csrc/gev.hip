// gev.hip -- KMATH_EIGEN_GEV (real A x = lambda B x; one GPU, or the 2-D cyclic blocks of a process grid) and its Cholesky-
// route range solver KMATH_EIGEN_GEV_RANGE (EXTENSION, one GPU).  Shared with the complex family (hgev.hip) through
// eigx_context.h: GevFrame, the test of B's smallest eigenvalue, dist_transpose and the SUMMA panel plan / packing.
#include "eigx_context.h"
#include "eigx_comm.h"
#include "../../include/eigenexa_amd.h"
#include <algorithm>

namespace eigx {

namespace {

// ---- KMATH_EIGEN_GEV: generalised symmetric-definite problem A x = lambda B x -----------------------------
// lower triangle := upper triangle (the GEMMs below need the full symmetric A; trpos_utol of the reference,
// src/KMATH_EIGEN_GEV_misc.F:140-173)
__global__ void symmetrize_kernel(double* __restrict__ a, int lda, int n) {
  const int j = blockIdx.y;
  for (int i = j + 1 + blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    a[(size_t)j * lda + i] = a[(size_t)i * lda + j];
}

// b(:, j) = z(:, k) * w(k)^(-1/2), k = n - 1 - j   (diag_mult, src/KMATH_EIGEN_GEV_misc.F:49-104, the columns in DESCENDING
// order of w).  A' = b^T A b is graded by w^(-1/2): in this order its large entries stand at the bottom right, where the
// reduction of eigen_s starts (it works from the last column up), and the small eigenvalues of A' come out to their own
// scale.  In ascending order they came out to eps |A'|: at cond(B) = 1e4 a hundred times the residual.
__global__ void scale_cols_rsqrt_reversed_kernel(const double* __restrict__ z, int ldz, const double* __restrict__ w,
                                                 double* __restrict__ b, int ldb, int n) {
  const int j = blockIdx.y, k = n - 1 - j;
  const double s = 1.0 / sqrt(w[k]);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    b[(size_t)j * ldb + i] = z[(size_t)k * ldz + i] * s;
}

// columns j and n - 1 - j of b change places (grid.y = n / 2)
__global__ void reverse_cols_kernel(double* __restrict__ b, int ldb, int n) {
  const int j = blockIdx.y, k = n - 1 - j;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const double t = b[(size_t)j * ldb + i];
    b[(size_t)j * ldb + i] = b[(size_t)k * ldb + i];
    b[(size_t)k * ldb + i] = t;
  }
}

// rows i and n - 1 - i of a change places in every column (grid.y = n)
__global__ void reverse_rows_kernel(double* __restrict__ a, int lda, int n) {
  double* col = a + (size_t)blockIdx.y * lda;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n / 2; i += gridDim.x * blockDim.x) {
    const double t = col[i];
    col[i] = col[n - 1 - i];
    col[n - 1 - i] = t;
  }
}

// ---- multi-rank KMATH_EIGEN_GEV on the 2-D cyclic blocks -------------------------------------------------------------
// (hgev.hip builds the complex generalised solver from the same transpose and panel packing: dist_transpose, summa_plan,
// summa_pack_a / summa_pack_b are declared in eigx_context.h)
// Two building blocks, both O(n^2 / P) memory per rank:
//   dist_transpose : Z = A^T.  Element A(j, i) lives on rank (j % Px, i % Py) and goes to rank (i % Px, j % Py): on a
//                    non-square grid that is a genuine all-to-all.  The rows i that rank (px, .) receives from a source in
//                    process column sy are the i = i0 + t L (L = lcm(Px, Py), i0 by the Chinese remainder theorem, none
//                    if px != sy mod gcd); likewise the columns j = j0 + u L: a piece is the (t, u) rectangle, piece
//                    [u][t].  (role of PDTRAN + trpos_utol, src/KMATH_EIGEN_GEV_1.F:57-58)
//   dist_gemm_nn   : C = A B (SUMMA): for every panel of kb global indices k the ranks of a process ROW allgather their
//                    columns of A(:, k-panel), the ranks of a process COLUMN their rows of B(k-panel, :), and the local
//                    fp64 MFMA GEMM accumulates the panel product.  (role of the three PDGEMMs, :100-139)
struct TrPeers { int i0[EIGX_MAXP], j0[EIGX_MAXP]; };   // per peer (world rank order): first row / column of the piece, -1 = empty
// pack: piece for destination d, element [u][t] = A(j0 + u L, i0 + t L) of my block (row j, column i)
__global__ void tr_pack_kernel(const double* __restrict__ a, int lda, int n, int Px, int Py, int L, TrPeers tp, int nimax,
                               int u0, int ucw, double* __restrict__ send) {
  const int d = blockIdx.z;
  const int i0 = tp.i0[d], j0 = tp.j0[d];
  for (int uu = blockIdx.y; uu < ucw; uu += gridDim.y) {
    const int u = u0 + uu;
    double* dst = send + ((size_t)d * ucw + uu) * nimax;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < nimax; t += gridDim.x * blockDim.x) {
      double v = 0.0;
      if (i0 >= 0 && j0 >= 0) {
        const int i = i0 + t * L, j = j0 + u * L;   // I hold row j (local j / Px), column i (local i / Py)
        if (i < n && j < n) v = a[(size_t)(i / Py) * lda + j / Px];
      }
      dst[t] = v;
    }
  }
}
// unpack: Z(i, j) = piece from source s at [u][t]; I hold row i (local i / Px), column j (local j / Py)
__global__ void tr_unpack_kernel(const double* __restrict__ recv, int n, int Px, int Py, int L, TrPeers tp, int nimax,
                                 int u0, int ucw, double* __restrict__ z, int ldz) {
  const int sidx = blockIdx.z;
  const int i0 = tp.i0[sidx], j0 = tp.j0[sidx];
  if (i0 < 0 || j0 < 0) return;
  for (int uu = blockIdx.y; uu < ucw; uu += gridDim.y) {
    const int u = u0 + uu;
    const double* src = recv + ((size_t)sidx * ucw + uu) * nimax;
    const int j = j0 + u * L;
    if (j >= n) return;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < nimax; t += gridDim.x * blockDim.x) {
      const int i = i0 + t * L;
      if (i < n) z[(size_t)(j / Py) * ldz + i / Px] = __hip_atomic_load(src + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}
static int crt_small(int a, int A_, int b, int B_, int L) {   // smallest x < L with x % A_ == a and x % B_ == b, -1 if none
  for (int x = 0; x < L; ++x)
    if (x % A_ == a && x % B_ == b) return x;
  return -1;
}
static int gcd_int(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }
// the pieces rank (px, py) exchanges with rank (qx, qy) in Z = A^T (pure arithmetic; eigx_transpose_plan exposes it to the
// CPU tests, which assemble A^T from the pieces for every grid)
static void transpose_plan(int Px, int Py, int px, int py, int qx, int qy, int* send_i0, int* send_j0, int* recv_i0,
                           int* recv_j0, int* step) {
  const int L = Px / gcd_int(Px, Py) * Py;
  // to (qx, qy): its rows i (i % Px == qx) among my columns (i % Py == py); its columns j (j % Py == qy) among my rows
  *send_i0 = crt_small(qx, Px, py, Py, L);
  *send_j0 = crt_small(px, Px, qy, Py, L);
  // from (qx, qy): my rows i (i % Px == px) among its columns (i % Py == qy); my columns j (j % Py == py) among its rows
  *recv_i0 = crt_small(px, Px, qy, Py, L);
  *recv_j0 = crt_small(qx, Px, py, Py, L);
  *step = L;
}

// a(i, j) for i > j (global indices) from t = a^T: the full symmetric matrix out of its upper triangle
__global__ void sym_merge_kernel(double* __restrict__ a, int lda, const double* __restrict__ t, int ldt, int nr, int Px, int px,
                                 int Py, int py) {
  const int lc = blockIdx.y, gj = lc * Py + py;
  for (int lr = blockIdx.x * blockDim.x + threadIdx.x; lr < nr; lr += gridDim.x * blockDim.x)
    if (lr * Px + px > gj) a[(size_t)lc * lda + lr] = t[(size_t)lc * ldt + lr];
}
// b(:, lc) = z(:, lc) * w(global column)^(-1/2) on the local block   (diag_mult, src/KMATH_EIGEN_GEV_misc.F:49-104)
__global__ void scale_cols_rsqrt_cyclic_kernel(const double* __restrict__ z, int ldz, const double* __restrict__ w,
                                               double* __restrict__ b, int ldb, int nr, int Py, int py) {
  const int lc = blockIdx.y;
  const double sc = 1.0 / sqrt(w[lc * Py + py]);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nr; i += gridDim.x * blockDim.x)
    b[(size_t)lc * ldb + i] = z[(size_t)lc * ldz + i] * sc;
}
// SUMMA panels.  A side: my columns lc0 .. lc0 + kbl - 1 of the panel, rows padded to nrp: out[c * nrp + r]
__global__ void mm_pack_a_kernel(const double* __restrict__ a, int lda, int nr, int nc, int lc0, int nrp, double* __restrict__ out) {
  const int c = blockIdx.y, lc = lc0 + c;
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < nrp; r += gridDim.x * blockDim.x)
    out[(size_t)c * nrp + r] = (r < nr && lc < nc) ? a[(size_t)lc * lda + r] : 0.0;
}
// B side: my rows lr0 .. lr0 + kbl - 1 of the panel for every local column j: out[j * kbl + rr]
__global__ void mm_pack_b_kernel(const double* __restrict__ b, int ldb, int nr, int nc, int lr0, int kbl, double* __restrict__ out) {
  const int j = blockIdx.y;
  for (int rr = blockIdx.x * blockDim.x + threadIdx.x; rr < kbl; rr += gridDim.x * blockDim.x)
    out[(size_t)j * kbl + rr] = (j < nc && lr0 + rr < nr) ? b[(size_t)j * ldb + lr0 + rr] : 0.0;
}
// gathered B rows [q'][j][rr] (k = k0 + rr Px + q') -> panel matrix Bp(pos, j) in the k order of the gathered A columns:
// k - k0 = c Py + q  ->  pos = q kbl_y + c
__global__ void mm_unpack_b_kernel(const double* __restrict__ recv, int Px, int Py, int kbl_x, int kbl_y, int ncp, int kb,
                                   double* __restrict__ Bp) {
  const int j = blockIdx.y, q = blockIdx.z;
  for (int rr = blockIdx.x * blockDim.x + threadIdx.x; rr < kbl_x; rr += gridDim.x * blockDim.x) {
    const int dk = rr * Px + q;
    Bp[(size_t)j * kb + (size_t)(dk % Py) * kbl_y + dk / Py] = recv[((size_t)q * ncp + j) * kbl_x + rr];
  }
}

}  // namespace

// ---- what the generalised drivers of both families share (eigx_context.h) ------------------------------------------------
int GevFrame::begin(bool args_ok) {
  if (!args_ok) return EIGX_ERR_BAD_ARG;
  EIGX_HIP_CHECK(hipSetDevice(ctx.device));
  EIGX_HIP_CHECK(hipStreamSynchronize(nullptr));   // the caller's default-stream work on the arguments (see SolveFrame::begin)
  t[0] = now_s();
  return EIGX_OK;
}
int GevFrame::finish() {
  mark();
  ctx.timers[0] = t[4] - t[0];
  for (int q = 1; q <= 4; ++q) ctx.timers[q] = t[q] - t[q - 1];
  return EIGX_OK;
}

int report_not_spd(const Context& ctx) {   // (w is replicated bit for bit on several ranks: all take the same way out)
  if (ctx.grid.rank == 0) fprintf(stderr, "[eigx] Matrix B is not positive definite!\n");   // src/KMATH_EIGEN_GEV_1.F:75-80
  return EIGX_ERR_NOT_SPD;
}
bool b_is_positive_definite(const Context& ctx, const double* w) {
  double wmin = 0.0;
  EIGX_HIP_CHECK(hipMemcpy(&wmin, w, 8, hipMemcpyDeviceToHost));
  if (!(wmin > 0.0)) report_not_spd(ctx);
  return wmin > 0.0;
}

// z(ldz, nc) = (a(lda, nc))^T on the cyclic blocks (both n x n); enqueued on st.  The all-to-all's pieces are uniform, and
// only gcd(Px, Py)^-2 of the rank pairs exchange anything, so the exchange runs in rounds over the pieces' columns u that
// keep the send + receive buffers (pool entries `tag`.tsend / `tag`.trecv) at about one local block each.
void dist_transpose(Context& ctx, int n, const double* a, int lda, double* z, int ldz, hipStream_t st, const char* tag) {
  const Grid& G = ctx.grid;
  const int g = gcd_int(G.Px, G.Py);
  const int P = G.nranks, L = G.Px / g * G.Py;
  const int nimax = ceil_div(n, L);
  const int ucw = ceil_div(nimax, g * g);                      // piece columns per round
  const size_t count = (size_t)nimax * ucw;
  double* sendb = ctx.pool.get_t<double>(std::string(tag) + ".tsend", count * P);
  double* recvb = ctx.pool.get_t<double>(std::string(tag) + ".trecv", count * P);
  TrPeers to, from;
  for (int q = 0; q < P; ++q) {
    const int qx = G.row_major ? q / G.Py : q % G.Px, qy = G.row_major ? q % G.Py : q / G.Px;
    int step_;
    transpose_plan(G.Px, G.Py, G.px, G.py, qx, qy, &to.i0[q], &to.j0[q], &from.i0[q], &from.j0[q], &step_);
  }
  const int gy = ucw < 32768 ? ucw : 32768;
  for (int u0 = 0; u0 < nimax; u0 += ucw) {
    hipLaunchKernelGGL(tr_pack_kernel, dim3(ceil_div(nimax, 256), gy, P), dim3(256), 0, st, a, lda, n, G.Px, G.Py, L, to, nimax, u0,
                       ucw, sendb);
    comm_exchange_big(ctx, COMM_WORLD, sendb, count, recvb, count, st);
    hipLaunchKernelGGL(tr_unpack_kernel, dim3(ceil_div(nimax, 256), gy, P), dim3(256), 0, st, (const double*)recvb, n, G.Px, G.Py, L,
                       from, nimax, u0, ucw, z, ldz);
  }
}

SummaPlan summa_plan(const Grid& G, int n, int kb_want) {
  const int nr = local_count(n, G.Px, G.px), nc = local_count(n, G.Py, G.py);
  const int L = G.Px / gcd_int(G.Px, G.Py) * G.Py, unit = 2 * L;   // panels start at multiples of Px and Py; even widths
  const int kb = unit * ceil_div(kb_want, unit);
  return {L, kb, kb / G.Px, kb / G.Py, ((nr > 2 ? nr : 2) + 1) & ~1, nc > 1 ? nc : 1};
}
void summa_pack_a(hipStream_t st, const SummaPlan& p, const double* a, int lda, int nr, int nc, int lc0, double* out) {
  hipLaunchKernelGGL(mm_pack_a_kernel, dim3(ceil_div(p.nrp, 256), p.kbl_y), dim3(256), 0, st, a, lda, nr, nc, lc0, p.nrp, out);
}
void summa_pack_b(hipStream_t st, const SummaPlan& p, const double* b, int ldb, int nr, int nc, int lr0, double* out) {
  hipLaunchKernelGGL(mm_pack_b_kernel, dim3(ceil_div(p.kbl_x, 256), p.ncp), dim3(256), 0, st, b, ldb, nr, nc, lr0, p.kbl_x, out);
}

namespace {

// C(ldc, nc) = A B on the cyclic blocks (all n x n, A and B complete -- not triangles); synchronous
static int dist_gemm_nn(Context& ctx, int n, const double* A, int lda, const double* B, int ldb, double* C, int ldc) {
  const Grid& G = ctx.grid;
  hipStream_t st = ctx.stream;
  const int nr = local_count(n, G.Px, G.px), nc = local_count(n, G.Py, G.py);
  // panel width: about n / 8 between 128 and 1024 (the panels are O(n kb / sqrt(P)) of workspace)
  const int kb_want = (n / 8 < 128) ? (n < 128 ? n : 128) : (n / 8 > 1024 ? 1024 : n / 8);
  const SummaPlan p = summa_plan(G, n, kb_want);
  const int kb = p.kb, kbl_x = p.kbl_x, kbl_y = p.kbl_y, nrp = p.nrp, ncp = p.ncp;
  double* sendA = ctx.pool.get_t<double>("gev.sa", (size_t)nrp * kbl_y);
  double* Ap = ctx.pool.get_t<double>("gev.pa", (size_t)nrp * kb);
  double* sendB = ctx.pool.get_t<double>("gev.sb", (size_t)kbl_x * ncp);
  double* recvB = ctx.pool.get_t<double>("gev.rb", (size_t)kb * ncp);
  double* Bp = ctx.pool.get_t<double>("gev.pb", (size_t)kb * ncp);
  for (int k0 = 0; k0 < n; k0 += kb) {
    summa_pack_a(st, p, A, lda, nr, nc, k0 / G.Py, sendA);
    comm_allgather(ctx, COMM_Y, sendA, Ap, (size_t)nrp * kbl_y, st);          // Ap(:, q kbl_y + c) = A(my rows, k0 + c Py + q)
    summa_pack_b(st, p, B, ldb, nr, nc, k0 / G.Px, sendB);
    comm_allgather(ctx, COMM_X, sendB, recvB, (size_t)kbl_x * ncp, st);
    hipLaunchKernelGGL(mm_unpack_b_kernel, dim3(ceil_div(kbl_x, 256), ncp, G.Px), dim3(256), 0, st, (const double*)recvB, G.Px, G.Py,
                       kbl_x, kbl_y, ncp, kb, Bp);
    if (nr > 0 && nc > 0) dgemm_dev(st, 'N', 'N', nr, nc, kb, 1.0, Ap, nrp, Bp, kb, k0 == 0 ? 0.0 : 1.0, C, ldc);
  }
  EIGX_HIP_CHECK(hipStreamSynchronize(st));
  return comm_failed(ctx) ? EIGX_ERR_INTERNAL : EIGX_OK;
}

// Same sequence as KMATH_EIGEN_GEV_1 (src/KMATH_EIGEN_GEV_1.F:57-139): eigen_s(B, 'X') -> B^(-1/2) := Z_B W_B^(-1/2);
// A' = B^(-1/2)^T A B^(-1/2) by two GEMMs; eigen_s(A', 'X') -> w, Y; Z = B^(-1/2) Y (B-orthonormal).  On entry only
// the upper triangles of a and b are significant; a, b are destroyed (a holds Y, b holds B^(-1/2) on exit, as in
// the reference).  One GPU; all three products run on the fp64 MFMA GEMM, and between the two solves the columns of
// B^(-1/2) stand in descending order of w (scale_cols_rsqrt_reversed_kernel says why); the several-rank path keeps the
// ascending order.
// Several ranks: the same sequence on the 2-D cyclic blocks, nothing gathered -- two distributed eigen_s solves, the
// symmetrisation of A and the transposed factor by dist_transpose, three SUMMA products with local MFMA GEMMs
// (round 4; the first version gathered A and B on every rank).
static int gev_dev_mg(Context& ctx, int n, double* a, int lda, double* b, int ldb, double* w, double* z, int ldz) {
  const Grid G = ctx.grid;
  const int nr = local_count(n, G.Px, G.px), nc = local_count(n, G.Py, G.py);
  const int lmin = nr > 1 ? nr : 1;
  GevFrame F(ctx);
  if (const int rc0 = F.begin(n > 0 && a && b && w && z && lda >= lmin && ldb >= lmin && ldz >= lmin)) return rc0;
  hipStream_t st = ctx.stream;
  const int ldt = pad_ld((nr > 2 ? nr : 2));
  const int ncd = nc > 0 ? nc : 1;
  double* tb = ctx.pool.get_t<double>("gev.t", (size_t)ldt * ncd);    // A^T, later (B^(-1/2))^T
  double* cb = ctx.pool.get_t<double>("gev.c", (size_t)ldt * ncd);    // C = A B^(-1/2)
  dist_transpose(ctx, n, a, lda, tb, ldt, st);
  if (nr > 0 && nc > 0)
    hipLaunchKernelGGL(sym_merge_kernel, dim3(ceil_div(nr, 256), nc), dim3(256), 0, st, a, lda, (const double*)tb, ldt, nr, G.Px, G.px,
                       G.Py, G.py);
  EIGX_HIP_CHECK(hipStreamSynchronize(st));
  if (comm_failed(ctx)) return EIGX_ERR_INTERNAL;
  int rc = solve_dev(ctx, n, n, b, ldb, w, z, ldz, 128, 128, 'X', 1, 1);      // B = Z_B W_B Z_B^T
  if (rc != EIGX_OK) return rc;
  F.mark();
  if (!b_is_positive_definite(ctx, w)) return EIGX_ERR_NOT_SPD;
  if (nr > 0 && nc > 0)
    hipLaunchKernelGGL(scale_cols_rsqrt_cyclic_kernel, dim3(ceil_div(nr, 256), nc), dim3(256), 0, st, (const double*)z, ldz,
                       (const double*)w, b, ldb, nr, G.Py, G.py);
  rc = dist_gemm_nn(ctx, n, a, lda, b, ldb, cb, ldt);                          // C  = A B^(-1/2)
  if (rc != EIGX_OK) return rc;
  dist_transpose(ctx, n, b, ldb, tb, ldt, st);                                 // (B^(-1/2))^T
  rc = dist_gemm_nn(ctx, n, tb, ldt, cb, ldt, z, ldz);                         // A' = B^(-1/2)^T C
  if (rc != EIGX_OK) return rc;
  F.mark();
  rc = solve_dev(ctx, n, n, z, ldz, w, a, lda, 128, 128, 'X', 1, 1);            // A' = Y W Y^T, Y in a
  if (rc != EIGX_OK) return rc;
  F.mark();
  rc = dist_gemm_nn(ctx, n, b, ldb, a, lda, z, ldz);                           // Z = B^(-1/2) Y
  if (rc != EIGX_OK) return rc;
  return F.finish();
}

int gev_dev(Context& ctx, int n, double* a, int lda, double* b, int ldb, double* w, double* z, int ldz) {
  if (!ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  if (ctx.grid.nranks != 1) return gev_dev_mg(ctx, n, a, lda, b, ldb, w, z, ldz);
  GevFrame F(ctx);
  if (const int rc0 = F.begin(n > 0 && a && b && w && z && lda >= n && ldb >= n && ldz >= n && !((lda | ldb | ldz) & 1))) return rc0;
  hipStream_t st = ctx.stream;
  hipLaunchKernelGGL(symmetrize_kernel, dim3(8, n), dim3(256), 0, st, a, lda, n);
  int rc = solve_dev(ctx, n, n, b, ldb, w, z, ldz, 128, 128, 'X', 1, 1);      // B = Z_B W_B Z_B^T
  if (rc != EIGX_OK) return rc;
  F.mark();
  if (!b_is_positive_definite(ctx, w)) return EIGX_ERR_NOT_SPD;
  hipLaunchKernelGGL(scale_cols_rsqrt_reversed_kernel, dim3(8, n), dim3(256), 0, st, z, ldz, w, b, ldb, n);
  const int ldc = pad_ld(n);
  double* c = ctx.pool.get_t<double>("gev.c", (size_t)ldc * n);
  dgemm_dev(st, 'N', 'N', n, n, n, 1.0, a, lda, b, ldb, 0.0, c, ldc);          // C  = A B^(-1/2)
  dgemm_dev(st, 'T', 'N', n, n, n, 1.0, b, ldb, c, ldc, 0.0, z, ldz);          // A' = B^(-1/2)^T C
  EIGX_HIP_CHECK(hipStreamSynchronize(st));
  F.mark();
  rc = solve_dev(ctx, n, n, z, ldz, w, a, lda, 128, 128, 'X', 1, 1);            // A' = Y W Y^T, Y in a
  if (rc != EIGX_OK) return rc;
  F.mark();
  dgemm_dev(st, 'N', 'N', n, n, n, 1.0, b, ldb, a, lda, 0.0, z, ldz);          // Z = B^(-1/2) Y
  if (n > 1) {   // on exit b and a are what the reference leaves: B^(-1/2) with its columns in ascending order of w, and its Y
    hipLaunchKernelGGL(reverse_cols_kernel, dim3(8, n / 2), dim3(256), 0, st, b, ldb, n);
    hipLaunchKernelGGL(reverse_rows_kernel, dim3(8, n), dim3(256), 0, st, a, lda, n);
  }
  EIGX_HIP_CHECK(hipStreamSynchronize(st));
  return F.finish();
}

int gev_host(Context& ctx, int n, double* a, int lda, double* b, int ldb, double* w, double* z, int ldz) {
  if (!ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  // host arrays: the rank's 2-D cyclic blocks a(lda, *), b(ldb, *), z(ldz, *) (one rank: the whole matrices)
  const int nr = local_count(n, ctx.grid.Px, ctx.grid.px), nc = local_count(n, ctx.grid.Py, ctx.grid.py);
  if (n <= 0 || !a || !b || !w || !z || lda < nr || ldb < nr || ldz < nr) return EIGX_ERR_BAD_ARG;
  const HostStage S(ctx, 8, nr, nc, a, lda, b, ldb, nc, n);
  const int rc = gev_dev(ctx, n, S.a, S.ldd, S.b, S.ldd, S.w, S.z, S.ldd);
  if (rc != EIGX_OK) return rc;   // nothing comes back, w included (hgev_host returns w in every case)
  S.w_back(w, n);
  S.back(z, ldz, S.z, nc);
  S.back(a, lda, S.a, nc);        // Y
  S.back(b, ldb, S.b, nc);        // B^(-1/2)
  return EIGX_OK;
}

// ---- KMATH_EIGEN_GEV_RANGE: eigenpairs il .. iu of A x = lambda B x by the Cholesky route (EXTENSION, one GPU) ----------
// B = U^T U (tri.hip) -> C = U^-T A U^-1 -> range_solve_dev(C, il, iu) on the eigen_sx route -> Z = U^-1 Y on the m
// columns.  n^3 / 3 + 2 n^3 + n^2 m flops through the MFMA GEMM where KMATH_EIGEN_GEV spends a whole eigen_s of B and
// 6 n^3.  B is not scaled: U carries sqrt of B's scale, C its inverse, and a B near the ends of the fp64 range
// overflows there (range_solve_dev scales C itself, but only once it has been formed).

// upper(c) = U^-T A U^-1 (below the diagonal c is unspecified); a is overwritten.  a: upper triangle significant.
// 5/3 n^3 flops: a <- U^-T sym(a), c = a^T, c <- U^-T c on the block columns that reach the upper triangle.
void gev_reduce_dev(Context& ctx, int n, double* a, int lda, const double* u, int ldu, const TriInv& V, double* c, int ldc) {
  hipStream_t st = ctx.stream;
  hipLaunchKernelGGL(symmetrize_kernel, dim3(8, n), dim3(256), 0, st, a, lda, n);
  trsm_upper_dev(ctx, 'T', n, n, u, ldu, a, lda, V);
  transpose_dev(st, n, a, lda, c, ldc);
  trsm_upper_dev(ctx, 'T', n, n, u, ldu, c, ldc, V, true);   // the solvers read the upper triangle only
}

}  // namespace

// W by value: the window goes to range_solve_dev on C as it is (B is not scaled, so the eigenvalues of C are the
// generalised ones; range_solve_dev applies its own sigma of C), m is read back for the back-substitution.
int gev_range_dev(Context& ctx, int n, RangeWindow W, double* a, int lda, double* b, int ldb, double* w, double* z, int ldz,
                  char mode) {
  if (!ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  if (ctx.grid.nranks != 1) return refuse_several_ranks(ctx);
  mode = upper_case(mode);
  GevFrame F(ctx);
  const bool even_ld = !((lda | ldb) & 1) && !(mode == 'A' && (ldz & 1));
  if (const int rc0 = F.begin(range_args_ok(n, W, a, lda, w, z, ldz, mode) && b && ldb >= n && even_ld)) return rc0;
  hipStream_t st = ctx.stream;
  const int wcap = range_w_cap(W, mode);
  // both significant triangles are scanned before anything is factored
  int rc = eigen_scaling(ctx, a, lda, false, n, w, nullptr, wcap);
  if (rc == EIGX_OK) rc = eigen_scaling(ctx, b, ldb, false, n, w, nullptr, wcap);
  if (rc != EIGX_OK) {
    if (W.by_value) *W.m_out = 0;
    return rc;
  }
  if (chol_upper_dev(ctx, n, b, ldb) != EIGX_OK) return report_not_spd(ctx);
  F.mark();
  const TriInv V = tri_inverses_dev(ctx, n, b, ldb);   // once per factor: the three solves below share them
  const int ldc = pad_ld(n);
  double* c = ctx.pool.get_t<double>("gevr.c", (size_t)ldc * n);
  gev_reduce_dev(ctx, n, a, lda, b, ldb, V, c, ldc);
  EIGX_HIP_CHECK(hipStreamSynchronize(st));
  F.mark();
  rc = range_solve_dev(ctx, n, W, c, ldc, w, z, ldz, 128, 128, mode, 2, false);
  if (rc != EIGX_OK) return rc;
  const int m = W.by_value ? *W.m_out : W.m();
  F.mark();
  if (mode == 'A' && m > 0) {
    trsm_upper_dev(ctx, 'N', n, m, b, ldb, z, ldz, V);   // Z = U^-1 Y
    EIGX_HIP_CHECK(hipStreamSynchronize(st));
  }
  return F.finish();
}

namespace {

int gev_range_host(Context& ctx, int n, RangeWindow W, double* a, int lda, double* b, int ldb, double* w, double* z, int ldz,
                   char mode) {
  return range_host_form(
      ctx, n, W, 8, a, lda, true, b, ldb, w, z, ldz, mode,
      [&](const HostStage& S) { return gev_range_dev(ctx, n, W, S.a, S.ldd, S.b, S.ldd, S.w, S.z, S.ldd, mode); },
      [&](const HostStage& S) { S.back(b, ldb, S.b, n); });   // U in the upper triangle; a is not returned
}

}  // namespace
}  // namespace eigx

using namespace eigx;

extern "C" {

int eigx_transpose_plan(int Px, int Py, int px, int py, int qx, int qy, int* send_i0, int* send_j0, int* recv_i0,
                        int* recv_j0, int* step) {
  if (Px < 1 || Py < 1 || px < 0 || px >= Px || py < 0 || py >= Py || qx < 0 || qx >= Px || qy < 0 || qy >= Py || !send_i0 ||
      !send_j0 || !recv_i0 || !recv_j0 || !step) return EIGX_ERR_BAD_ARG;
  transpose_plan(Px, Py, px, py, qx, qy, send_i0, send_j0, recv_i0, recv_j0, step);
  return EIGX_OK;
}

int eigx_gev(int n, double* a, int lda, double* b, int ldb, double* w, double* z, int ldz) {
  return eigx_guard(g_ctx, [&] { return gev_host(g_ctx, n, a, lda, b, ldb, w, z, ldz); });
}
int eigx_gev_dev(int n, double* a, int lda, double* b, int ldb, double* w, double* z, int ldz) {
  return eigx_guard(g_ctx, [&] { return gev_dev(g_ctx, n, a, lda, b, ldb, w, z, ldz); });
}

// EXTENSION: eigenpairs il .. iu of A x = lambda B x by the Cholesky route (one GPU); see gev_range_dev
int eigx_gev_range(int n, int il, int iu, double* a, int lda, double* b, int ldb, double* w, double* z, int ldz, char mode) {
  return eigx_guard(g_ctx, [&] { return gev_range_host(g_ctx, n, RangeWindow::index(il, iu), a, lda, b, ldb, w, z, ldz, mode); });
}
int eigx_gev_range_dev(int n, int il, int iu, double* a, int lda, double* b, int ldb, double* w, double* z, int ldz, char mode) {
  return eigx_guard(g_ctx, [&] { return gev_range_dev(g_ctx, n, RangeWindow::index(il, iu), a, lda, b, ldb, w, z, ldz, mode); });
}
// the same for the eigenpairs with vl <= lambda < vu
int eigx_gev_range_v(int n, double vl, double vu, int mmax, int* m, int* il, double* a, int lda, double* b, int ldb, double* w,
                     double* z, int ldz, char mode) {
  return eigx_guard(g_ctx, [&] {
    return gev_range_host(g_ctx, n, RangeWindow::value(vl, vu, mmax, m, il), a, lda, b, ldb, w, z, ldz, mode);
  });
}
int eigx_gev_range_v_dev(int n, double vl, double vu, int mmax, int* m, int* il, double* a, int lda, double* b, int ldb,
                         double* w, double* z, int ldz, char mode) {
  return eigx_guard(g_ctx, [&] {
    return gev_range_dev(g_ctx, n, RangeWindow::value(vl, vu, mmax, m, il), a, lda, b, ldb, w, z, ldz, mode);
  });
}
// its reduction stage alone: upper(a) <- U^-T A U^-1 (all of a is written)
int eigx_gev_reduce_dev(int n, double* a_dev, int lda, const double* u_dev, int ldu) {
  if (!g_ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  if (n <= 0 || !a_dev || !u_dev || lda < n || ldu < n) return EIGX_ERR_BAD_ARG;
  if (g_ctx.grid.nranks != 1) return EIGX_ERR_INTERNAL;
  return eigx_guard(g_ctx, [&] {
    EIGX_HIP_CHECK(hipSetDevice(g_ctx.device));
    EIGX_HIP_CHECK(hipStreamSynchronize(nullptr));
    const TriInv V = tri_inverses_dev(g_ctx, n, u_dev, ldu);
    const int ldc = pad_ld(n);
    double* c = g_ctx.pool.get_t<double>("gevr.c", (size_t)ldc * n);
    gev_reduce_dev(g_ctx, n, a_dev, lda, u_dev, ldu, V, c, ldc);
    EIGX_HIP_CHECK(hipMemcpy2DAsync(a_dev, (size_t)lda * 8, c, (size_t)ldc * 8, (size_t)n * 8, (size_t)n, hipMemcpyDeviceToDevice,
                                    g_ctx.stream));
    EIGX_HIP_CHECK(hipStreamSynchronize(g_ctx.stream));
    return EIGX_OK;
  });
}

}  // extern "C"
