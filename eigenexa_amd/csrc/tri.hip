// tri.hip -- triangular stages of the Cholesky-route generalised solver (EXTENSION, one GPU; LAPACK uplo = 'U').
//   chol_upper_dev    : B = U^T U, U in place in the upper triangle (role of dpotrf)
//   tri_inverses_dev  : the inverses of the NB-wide diagonal blocks of U (pool buffer gevr.inv)
//   trsm_upper_dev    : X <- op(U)^-1 X by block inversion (role of dtrsm, side = 'L')
//   transpose_dev     : out = in^T
// NB is the outer block width (eigx_tune key 20).  Everything of O(n^3) runs in the fp64 MFMA GEMM (dgemm_dev):
//   Cholesky: per outer panel ONE trailing update with K = NB on the tiles of the upper triangle (tri_mode 1); inside a
//             panel 64-wide steps: diagonal block (one wave, column per lane in registers), its row panel
//             U12 = U11^-T B12 (64 x 64 tiles, the inverse of the diagonal block from LDS), a K = 64 update of the
//             panel's remaining rows.
//   solve   : inv(U_kk) of the NB-wide diagonal blocks once per factor -- 64 x 64 blocks inverted in ONE batched launch,
//             widths doubled by inv([U11 U12; 0 U22]) = [V11, -V11 U12 V22; 0 V22] with batched GEMMs -- then per block
//             row X_k <- V_kk X_k and X_rest <- X_rest - U_{k,rest}^T X_k: two GEMMs with K = NB.
// Nothing below the diagonal of B / U is read; what the kernels write there is unspecified.
// The m x m helpers of the Rayleigh-Ritz stage (subset.hip: cholesky_dev / trsm_right_dev) are a different, lower-
// triangular pair and stay as they are.
#include "eigx_context.h"
#include "../../include/eigenexa_amd.h"
#include <algorithm>
#include <cfloat>

namespace eigx {

namespace {

constexpr int TB = 64;   // inner block = one wave, one column per lane
int g_tri_nb = 256;      // eigx_tune key 20

// S[i][c] = block(i, c) for i <= c < nb, the identity beyond nb, zero below the diagonal.  One wave; a column per step,
// lanes along the rows (coalesced), LDS rows padded by one (conflict-free in both directions).
__device__ inline void load_upper64(double (*S)[TB + 1], const double* __restrict__ src, int ld, int nb, int lane) {
  for (int c = 0; c < TB; ++c)
    S[lane][c] = (lane <= c && c < nb) ? src[(size_t)c * ld + lane] : (lane == c ? 1.0 : 0.0);
}

// Right-looking U^T U factorisation of a 64 x 64 block held as c[i] = element (i, lane).  The scaled row k goes through
// LDS (double-buffered: one barrier per step); entries below the diagonal take part as dead weight and are never read
// as part of U.  Returns true on a pivot that is not > 0 or not finite (the pivot is replaced by 1).
__device__ inline bool chol64_wave(double (&c)[TB], double* row, int lane) {
  bool bad = false;
#pragma unroll
  for (int k = 0; k < TB; ++k) {
    double* r = row + (k & 1) * TB;
    r[lane] = c[k];
    __syncthreads();
    const double d = r[k];
    double s = 1.0;
    if (!(d > 0.0) || !(d <= DBL_MAX)) bad = true;
    else s = sqrt(d);
    const double rinv = 1.0 / s;
    const double ck = (lane == k) ? s : c[k] * rinv;
    c[k] = ck;
#pragma unroll
    for (int i = k + 1; i < TB; ++i) c[i] -= (r[i] * rinv) * ck;
  }
  return bad;
}

// Column `lane` of the inverse of the upper triangular S (zero below the diagonal) by back substitution; the row of S is a
// broadcast read.
__device__ inline void inv64_wave(const double (*S)[TB + 1], double (&v)[TB], int lane) {
#pragma unroll
  for (int i = TB - 1; i >= 0; --i) {
    double s = (i == lane) ? 1.0 : 0.0;
#pragma unroll
    for (int k = i + 1; k < TB; ++k) s -= S[i][k] * v[k];
    v[i] = s / S[i][i];
  }
}

// Diagonal block [k0, k0 + nb) of the Cholesky factorisation: U_kk in place, and Vt = its inverse, ROW-major 64 x 64
// (Vt[k * 64 + i] = inv(U_kk)(k, i)), as chol_row_panel_kernel reads it.  stat[0] = 1 on a breakdown.
__global__ __launch_bounds__(TB) void chol_diag_upper_kernel(double* __restrict__ B, int ldb, int k0, int nb,
                                                             double* __restrict__ Vt, int* __restrict__ stat) {
  __shared__ double S[TB][TB + 1];
  __shared__ double row[2 * TB];
  const int lane = threadIdx.x;
  double* blk = B + (size_t)k0 * ldb + k0;
  load_upper64(S, blk, ldb, nb, lane);
  __syncthreads();
  double c[TB];
#pragma unroll
  for (int i = 0; i < TB; ++i) c[i] = S[i][lane];
  const bool bad = chol64_wave(c, row, lane);
  __syncthreads();
#pragma unroll
  for (int i = 0; i < TB; ++i) S[i][lane] = (i <= lane) ? c[i] : 0.0;
  __syncthreads();
  for (int q = 0; q < nb; ++q)
    if (lane <= q) blk[(size_t)q * ldb + lane] = S[lane][q];
  double v[TB];
  inv64_wave(S, v, lane);
#pragma unroll
  for (int i = 0; i < TB; ++i) Vt[i * TB + lane] = v[i];
  if (bad && lane == 0) stat[0] = 1;
}

// Row panel of one 64-wide step: B(k0 : k0 + nb, c0 + 64 t : ...) <- inv(U_kk)^T B(...), one 64 x 64 tile per workgroup.
// out(i, c) = sum_k V(k, i) T(k, c): thread = row i, a wave = 16 columns; V(k, .) is read along the lanes, T(k, c) is a
// broadcast.
__global__ __launch_bounds__(256) void chol_row_panel_kernel(double* __restrict__ B, int ldb, int k0, int nb, int c0, int ncols,
                                                             const double* __restrict__ Vt) {
  __shared__ double Vs[TB * TB];   // Vs[k * 64 + i] = V(k, i)
  __shared__ double Ts[TB * TB];   // Ts[c * 64 + k] = B(k0 + k, c0 + cb + c)
  const int tid = threadIdx.x;
  const int cb = blockIdx.x * TB;
  for (int q = tid; q < TB * TB; q += 256) {
    const int k = q & (TB - 1), c = q >> 6;
    Vs[q] = Vt[q];
    Ts[q] = (k < nb && cb + c < ncols) ? B[(size_t)(c0 + cb + c) * ldb + k0 + k] : 0.0;
  }
  __syncthreads();
  const int i = tid & (TB - 1), cw = (tid >> 6) * 16;
  double acc[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) acc[t] = 0.0;
  for (int k = 0; k < TB; ++k) {
    const double v = Vs[k * TB + i];
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[t] += v * Ts[(cw + t) * TB + k];
  }
  if (i < nb) {
#pragma unroll
    for (int t = 0; t < 16; ++t)
      if (cb + cw + t < ncols) B[(size_t)(c0 + cb + cw + t) * ldb + k0 + i] = acc[t];
  }
}

// Inverses of all 64-wide diagonal blocks of U in one launch (block q of the grid: rows / columns [64 q, 64 q + 64)),
// written to their place inside the NB x NB inverse of outer block 64 q / NB (column-major, leading dimension NB).
__global__ __launch_bounds__(TB) void tri_inv_diag_kernel(const double* __restrict__ U, int ldu, int n, int NB,
                                                          double* __restrict__ Vinv) {
  __shared__ double S[TB][TB + 1];
  const int lane = threadIdx.x;
  const int k0 = blockIdx.x * TB, nb = (n - k0 < TB) ? n - k0 : TB;
  load_upper64(S, U + (size_t)k0 * ldu + k0, ldu, nb, lane);
  __syncthreads();
  double v[TB];
  inv64_wave(S, v, lane);
  __syncthreads();
#pragma unroll
  for (int i = 0; i < TB; ++i) S[i][lane] = v[i];
  __syncthreads();
  const int K = k0 / NB, off = k0 - K * NB;
  double* dst = Vinv + (size_t)K * NB * NB + (size_t)off * NB + off;
  for (int q = 0; q < nb; ++q)
    if (lane < nb) dst[(size_t)q * NB + lane] = S[lane][q];
}

__global__ __launch_bounds__(256) void transpose_kernel(const double* __restrict__ in, int ldi, double* __restrict__ out, int ldo,
                                                        int n) {
  __shared__ double T[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int r0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  for (int c = ty; c < 32; c += 8)
    if (r0 + tx < n && c0 + c < n) T[c][tx] = in[(size_t)(c0 + c) * ldi + r0 + tx];
  __syncthreads();
  for (int c = ty; c < 32; c += 8)
    if (c0 + tx < n && r0 + c < n) out[(size_t)(r0 + c) * ldo + c0 + tx] = T[tx][c];
}

}  // namespace

// key 20: outer block width of the triangular stages, a multiple of 64 from 64 to 1024; another value is refused (-1)
int set_tri_nb(int v) {
  if (v < 64 || v > 1024 || (v % 64) != 0) return -1;
  const int old = g_tri_nb;
  g_tri_nb = v;
  return old;
}
int get_tri_nb() { return g_tri_nb; }

void transpose_dev(hipStream_t st, int n, const double* in, int ldi, double* out, int ldo) {
  const int t = ceil_div(n, 32);
  hipLaunchKernelGGL(transpose_kernel, dim3(t, t), dim3(256), 0, st, in, ldi, out, ldo, n);
}

int chol_upper_dev(Context& ctx, int n, double* B, int ldb) {
  hipStream_t st = ctx.stream;
  const int NB = g_tri_nb;
  int* stat = ctx.pool.get_t<int>("gevr.stat", 4);
  double* Vt = ctx.pool.get_t<double>("gevr.v64", (size_t)TB * TB);
  EIGX_HIP_CHECK(hipMemsetAsync(stat, 0, 4 * sizeof(int), st));
  for (int p0 = 0; p0 < n; p0 += NB) {
    const int p1 = std::min(p0 + NB, n);
    for (int j0 = p0; j0 < p1; j0 += TB) {
      const int nb = std::min(TB, n - j0), j1 = j0 + nb;
      hipLaunchKernelGGL(chol_diag_upper_kernel, dim3(1), dim3(TB), 0, st, B, ldb, j0, nb, Vt, stat);
      if (j1 >= n) break;
      hipLaunchKernelGGL(chol_row_panel_kernel, dim3(ceil_div(n - j1, TB)), dim3(256), 0, st, B, ldb, j0, nb, j1, n - j1,
                         (const double*)Vt);
      // the panel's remaining rows, all columns to the right: B(j1:p1, j1:n) -= U(j0:j1, j1:p1)^T U(j0:j1, j1:n)
      const double* Urow = B + (size_t)j1 * ldb + j0;
      if (j1 < p1) dgemm_dev(st, 'T', 'N', p1 - j1, n - j1, nb, -1.0, Urow, ldb, Urow, ldb, 1.0, B + (size_t)j1 * ldb + j1, ldb);
    }
    if (p1 < n) {
      // trailing update of the outer panel, tiles of the upper triangle only
      const double* Up = B + (size_t)p1 * ldb + p0;
      dgemm_dev(st, 'T', 'N', n - p1, n - p1, p1 - p0, -1.0, Up, ldb, Up, ldb, 1.0, B + (size_t)p1 * ldb + p1, ldb, 1);
    }
  }
  int bad = 0;
  EIGX_HIP_CHECK(hipMemcpyAsync(&bad, stat, sizeof(int), hipMemcpyDeviceToHost, st));
  EIGX_HIP_CHECK(hipStreamSynchronize(st));
  return bad ? EIGX_ERR_NOT_SPD : EIGX_OK;
}

TriInv tri_inverses_dev(Context& ctx, int n, const double* U, int ldu) {
  hipStream_t st = ctx.stream;
  const int NB = g_tri_nb;
  const int nblk = ceil_div(n, NB), nfull = n / NB, Wl = n - nfull * NB;
  TriInv V;
  V.nb = NB;
  V.v = ctx.pool.get_t<double>("gevr.inv", (size_t)nblk * NB * NB);
  // U12 V22 of one level: at most n / (2 w) blocks of w x w, w < NB
  double* T = ctx.pool.get_t<double>("gevr.invt", (size_t)n * NB + (size_t)NB * NB);
  EIGX_HIP_CHECK(hipMemsetAsync(V.v, 0, (size_t)nblk * NB * NB * sizeof(double), st));
  hipLaunchKernelGGL(tri_inv_diag_kernel, dim3(ceil_div(n, TB)), dim3(TB), 0, st, U, ldu, n, NB, V.v);
  // `batch` pairs (left block of width w at local offset o + 2 w q, right block of width wr behind it) in each of `batch2`
  // outer blocks from K0 on: V12 = -V11 (U12 V22)
  auto pairs = [&](int K0, int o, int w, int wr, int batch, int batch2) {
    if (batch <= 0 || batch2 <= 0 || wr <= 0) return;
    const size_t r0 = (size_t)K0 * NB + o;
    const double* U12 = U + r0 + (r0 + w) * ldu;
    double* Vb = V.v + (size_t)K0 * NB * NB;
    const double* V11 = Vb + o + (size_t)o * NB;
    const double* V22 = Vb + (o + w) + (size_t)(o + w) * NB;
    double* V12 = Vb + o + (size_t)(o + w) * NB;
    const long sU = 2L * w * (ldu + 1), sV = 2L * w * (NB + 1), sT = (long)w * w;
    const long sU2 = (long)NB * (ldu + 1), sV2 = (long)NB * NB, sT2 = sT * batch;
    dgemm_dev(st, 'N', 'N', w, wr, wr, 1.0, U12, ldu, V22, NB, 0.0, T, w, 0, nullptr, nullptr, nullptr, batch, sU, sV, sT, batch2,
              sU2, sV2, sT2);
    dgemm_dev(st, 'N', 'N', w, wr, w, -1.0, V11, NB, T, w, 0.0, V12, NB, 0, nullptr, nullptr, nullptr, batch, sV, sT, sV, batch2,
              sV2, sT2, sV2);
  };
  for (int w = TB; w < NB; w *= 2) {
    const int npf = NB / (2 * w), rem = NB - npf * 2 * w;       // the full outer blocks
    pairs(0, 0, w, w, npf, nfull);
    if (rem > w) pairs(0, npf * 2 * w, w, rem - w, 1, nfull);
    const int npl = Wl / (2 * w), reml = Wl - npl * 2 * w;      // the last, narrower one
    pairs(nfull, 0, w, w, npl, 1);
    if (reml > w) pairs(nfull, npl * 2 * w, w, reml - w, 1, 1);
  }
  return V;
}

void trsm_upper_dev(Context& ctx, char trans, int n, int nrhs, const double* U, int ldu, double* X, int ldx, const TriInv& V,
                    bool upper_only) {
  if (nrhs <= 0) return;
  if (trans != 'T' || nrhs != n) upper_only = false;
  hipStream_t st = ctx.stream;
  const int NB = V.nb, nblk = ceil_div(n, NB);
  double* tmp = ctx.pool.get_t<double>("gevr.xk", (size_t)NB * nrhs);
  for (int q = 0; q < nblk; ++q) {
    const int K = (trans == 'T') ? q : nblk - 1 - q;           // U^T is lower triangular: forwards; U: backwards
    const int k0 = K * NB, w = std::min(NB, n - k0), k1 = k0 + w;
    // upper_only (trans 'T', X square): block row K of the result is wanted from column k0 on, and the rows below it want
    // still fewer columns, so the columns before k0 drop out of this and every later step (2/3 of the flops remain)
    const int c0 = upper_only ? k0 : 0, nc = nrhs - c0;
    double* Xc = X + (size_t)c0 * ldx;
    const double* Vk = V.v + (size_t)K * NB * NB;
    dgemm_dev(st, trans, 'N', w, nc, w, 1.0, Vk, NB, Xc + k0, ldx, 0.0, tmp, NB);
    EIGX_HIP_CHECK(hipMemcpy2DAsync(Xc + k0, (size_t)ldx * 8, tmp, (size_t)NB * 8, (size_t)w * 8, (size_t)nc,
                                    hipMemcpyDeviceToDevice, st));
    if (trans == 'T') {
      if (k1 < n) dgemm_dev(st, 'T', 'N', n - k1, nc, w, -1.0, U + (size_t)k1 * ldu + k0, ldu, tmp, NB, 1.0, Xc + k1, ldx);
    } else {
      if (k0 > 0) dgemm_dev(st, 'N', 'N', k0, nc, w, -1.0, U + (size_t)k0 * ldu, ldu, tmp, NB, 1.0, Xc, ldx);
    }
  }
}

}  // namespace eigx

using namespace eigx;

extern "C" {

int eigx_chol_dev(int n, double* b_dev, int ldb) {
  if (!g_ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  if (n <= 0 || !b_dev || ldb < n) return EIGX_ERR_BAD_ARG;
  if (g_ctx.grid.nranks != 1) return EIGX_ERR_INTERNAL;
  return eigx_guard(g_ctx, [&] {
    EIGX_HIP_CHECK(hipSetDevice(g_ctx.device));
    EIGX_HIP_CHECK(hipStreamSynchronize(nullptr));
    return chol_upper_dev(g_ctx, n, b_dev, ldb);
  });
}

int eigx_trsm_upper_dev(char trans, int n, int nrhs, const double* u_dev, int ldu, double* x_dev, int ldx) {
  if (!g_ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  trans = upper_case(trans);
  if (n <= 0 || nrhs < 0 || !u_dev || !x_dev || ldu < n || ldx < n || (trans != 'N' && trans != 'T')) return EIGX_ERR_BAD_ARG;
  if (g_ctx.grid.nranks != 1) return EIGX_ERR_INTERNAL;
  return eigx_guard(g_ctx, [&] {
    EIGX_HIP_CHECK(hipSetDevice(g_ctx.device));
    EIGX_HIP_CHECK(hipStreamSynchronize(nullptr));
    const TriInv V = tri_inverses_dev(g_ctx, n, u_dev, ldu);
    trsm_upper_dev(g_ctx, trans, n, nrhs, u_dev, ldu, x_dev, ldx, V, false);
    EIGX_HIP_CHECK(hipStreamSynchronize(g_ctx.stream));
    return EIGX_OK;
  });
}

}  // extern "C"
