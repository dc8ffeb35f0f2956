// subset.hip -- eigenvectors of the symmetric band matrix (band = 1 tridiagonal, 2 pentadiagonal) for a CHOSEN set of
// eigenvalues, gfx950, one GPU.  EXTENSION: the reference has no index-range interface (its eigen_sx / eigen_s always run
// the divide and conquer for all n eigenvectors and trim afterwards, src/eigen_sx.F:200-240).
//
// Work and memory are proportional to the number m of wanted eigenpairs:
//   1. inverse iteration on T - lambda_j I, ONE EIGENVECTOR PER THREAD: banded LU with partial pivoting (fill-in: band
//      extra super-diagonals), a random start that is back-substituted directly and two full solve-and-normalise
//      sweeps (three back-substitutions).  Exact zero pivots become
//      eps ||T|| (DLAGTF), eigenvalues closer than 10 eps ||T|| are nudged apart first (DSTEIN).  Factor and vectors
//      are stored with the vector index fastest (element i of vector j at i * stride + j): the 64 lanes of a wave touch
//      one contiguous line per step.  Columns are processed in chunks so that the scratch stays bounded.
//   2. block orthonormalisation by CholQR2 (Gram matrix, blocked Cholesky on the device, triangular solve) and
//      Rayleigh-Ritz: H = Q^T (T Q), the dense m x m problem goes through the library's own reduction / divide and
//      conquer / back-transformation, Z = Q S.  All O(n m^2) work is fp64 MFMA GEMM (dgemm_dev).  This replaces DSTEIN's
//      serial per-cluster Gram-Schmidt and restores orthogonality when the whole window is one cluster.
//   3. acceptance test: the result is refused (positive return) when a Cholesky factorisation breaks down or the
//      conditioning estimate max / min diag(L) of the first one exceeds 10^key19 (default 1e6; CholQR2 is safe to about
//      eps^-1/2).  The range driver (solver.hip) then falls back to the full divide and conquer.
// The inner m x m solve re-enters band_reduce_dev / band_dc_dev / trbak_dev, whose pooled buffers are shared by name: the
// caller's d / e must not live in a "red.", "dc." or "bt." buffer, and the caller prepares its own back-transformation
// AFTER this stage (range_solve_dev does).
#include "eigx_context.h"
#include "../../include/eigenexa_amd.h"
#include <algorithm>
#include <cfloat>
#include <limits>
#include <vector>

namespace eigx {

namespace {

// eigx_tune key 17: windows with 100 m > pct n go straight to the full divide and conquer.  -1 = automatic, from the measured
// table: 10 % from n = 32768 on (not slower up to m / n = 12.5 % there), 3 % from n = 16384 on (not slower
// at 3.1 %, slower at 25 %), 0 below (at n = 8192 the subset path was slower at every m)
int g_range_pct = -1;
inline int range_auto_pct(int n) { return n >= 32768 ? 10 : (n >= 16384 ? 3 : 0); }
int g_range_optin = 0;     // key 18: eigx_sx / eigx_s with 0 < nvec < n take the range path
int g_range_logcond = 6;   // key 19: log10 of the acceptance bound on cond(L)
RangeInfo g_range_info = {0, 0, 0.0, {0.0, 0.0, 0.0, 0.0}};

constexpr int II_SWEEPS = 3;

struct IIArgs {
  int n, lde;
  const double* d; const double* e;
  const double* lam;     // [mc] shifts of this chunk (sorted, nudged apart)
  int mc, stride;        // columns of the chunk, their padded count (distance between consecutive rows in the scratch)
  int j0;                // global index of the chunk's first column (seeds the start vectors)
  double* U;             // [n][2 band + 1][stride]: 1 / pivot, then the 2 band entries right of it
  double* L;             // [n][band][stride] multipliers
  unsigned char* P;      // [n][stride] pivot row offset (0 .. band)
  double* X; double* Y;  // [n][stride] each: iterate / forward-solved right-hand side
  double* amax;          // [stride] max |x| of the last sweep
  double eps_t;          // eps ||T||: replaces an exact zero pivot
};

// T(i, i + off) of the band matrix (zero outside the matrix); e(i, b) = T(i - b, i)
template <int B>
__device__ __forceinline__ double band_entry(const IIArgs& a, int i, int off) {
  if (i < 0 || i >= a.n) return 0.0;
  if (off == 0) return a.d[i];
  if (off > 0) return (i + off < a.n) ? a.e[(size_t)(off - 1) * a.lde + i + off] : 0.0;
  return (i + off >= 0) ? a.e[(size_t)(-off - 1) * a.lde + i] : 0.0;
}

__device__ __forceinline__ double start_value(unsigned i, unsigned j) {   // seeded pseudo-random start in [-1, 1)
  unsigned long long z = ((unsigned long long)j << 32 | i) + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (double)(long long)(z >> 11) * 0x1p-52 - 1.0;
}

// One thread = one eigenvector.  Window W[r][c] of the partially eliminated rows k .. k + B, columns k .. k + 2 B, in
// registers; everything that depends on the row index only (d, e) is wave-uniform.
template <int B>
__global__ __launch_bounds__(64) void inviter_kernel(IIArgs a) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= a.mc) return;
  constexpr int WC = 2 * B + 1;
  const int n = a.n;
  const size_t sd = (size_t)a.stride;
  const double lam = a.lam[j];
  double* __restrict__ U = a.U + j;
  double* __restrict__ Lm = a.L + j;
  unsigned char* __restrict__ Pv = a.P + j;
  double* __restrict__ X = a.X + j;
  double* __restrict__ Y = a.Y + j;

  // ---- factorisation P (T - lam I) = L U -------------------------------------------------------------------------
  double W[B + 1][WC];
#pragma unroll
  for (int r = 0; r <= B; ++r)
#pragma unroll
    for (int c = 0; c < WC; ++c) {
      const int off = c - r;
      W[r][c] = (off <= B && c < n) ? band_entry<B>(a, r, off) - (off == 0 ? lam : 0.0) : 0.0;
    }
  for (int k = 0; k < n; ++k) {
    int p = 0;
    double best = fabs(W[0][0]);
#pragma unroll
    for (int r = 1; r <= B; ++r)
      if (fabs(W[r][0]) > best) { best = fabs(W[r][0]); p = r; }
#pragma unroll
    for (int r = 1; r <= B; ++r)
      if (p == r) {
#pragma unroll
        for (int c = 0; c < WC; ++c) { const double t = W[0][c]; W[0][c] = W[r][c]; W[r][c] = t; }
      }
    double piv = W[0][0];
    if (piv == 0.0) piv = a.eps_t;
    const double rinv = 1.0 / piv;
    double* Uk = U + (size_t)k * WC * sd;
    Uk[0] = rinv;
#pragma unroll
    for (int c = 1; c < WC; ++c) Uk[(size_t)c * sd] = W[0][c];
    Pv[(size_t)k * sd] = (unsigned char)p;
#pragma unroll
    for (int r = 1; r <= B; ++r) {
      const double l = W[r][0] * rinv;
      Lm[((size_t)k * B + (r - 1)) * sd] = l;
#pragma unroll
      for (int c = 1; c < WC; ++c) W[r][c] -= l * W[0][c];
    }
    // the window moves one row down and one column right; row k + B + 1 enters with its whole band
#pragma unroll
    for (int r = 0; r < B; ++r) {
#pragma unroll
      for (int c = 0; c < WC - 1; ++c) W[r][c] = W[r + 1][c + 1];
      W[r][WC - 1] = 0.0;
    }
    const int in = k + B + 1;
#pragma unroll
    for (int c = 0; c < WC; ++c) W[B][c] = band_entry<B>(a, in, c - B) - ((c == B && in < n) ? lam : 0.0);
  }

  // ---- sweeps: the first one back-substitutes the random start directly (L y = b with b random) ------------------
  double scale = 1.0, amax = 0.0;
  for (int sweep = 0; sweep < II_SWEEPS; ++sweep) {
    if (sweep > 0) {
      // forward: y = L^-1 P (x * scale)
      double xw[B + 1];
#pragma unroll
      for (int r = 0; r <= B; ++r) xw[r] = (r < n) ? X[(size_t)r * sd] * scale : 0.0;
      for (int k = 0; k < n; ++k) {
        const int p = Pv[(size_t)k * sd];
#pragma unroll
        for (int r = 1; r <= B; ++r)
          if (p == r) { const double t = xw[0]; xw[0] = xw[r]; xw[r] = t; }
        const double y = xw[0];
        Y[(size_t)k * sd] = y;
#pragma unroll
        for (int r = 1; r <= B; ++r) xw[r] -= Lm[((size_t)k * B + (r - 1)) * sd] * y;
#pragma unroll
        for (int r = 0; r < B; ++r) xw[r] = xw[r + 1];
        const int in = k + B + 1;
        xw[B] = (in < n) ? X[(size_t)in * sd] * scale : 0.0;
      }
    }
    // backward: x = U^-1 y
    double s[2 * B];
#pragma unroll
    for (int c = 0; c < 2 * B; ++c) s[c] = 0.0;
    amax = 0.0;
    for (int k = n - 1; k >= 0; --k) {
      const double* Uk = U + (size_t)k * WC * sd;
      double v = (sweep > 0) ? Y[(size_t)k * sd] : start_value((unsigned)k, (unsigned)(a.j0 + j));
#pragma unroll
      for (int c = 1; c < WC; ++c) v -= Uk[(size_t)c * sd] * s[c - 1];
      v *= Uk[0];
#pragma unroll
      for (int c = 2 * B - 1; c > 0; --c) s[c] = s[c - 1];
      s[0] = v;
      X[(size_t)k * sd] = v;
      amax = fmax(amax, fabs(v));
    }
    scale = (amax > 0.0 && amax <= DBL_MAX) ? 1.0 / amax : 1.0;
  }
  a.amax[j] = amax;
}

// Yout(i, j0 + j) = X[i][j] / amax[j]  (vector-fastest scratch -> column-major), 32 x 32 tiles through LDS
__global__ __launch_bounds__(256) void ii_transpose_kernel(const double* __restrict__ X, const double* __restrict__ amax,
                                                           int n, int mc, int stride, double* __restrict__ Yout, int ldy) {
  __shared__ double tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
  const int i0 = blockIdx.x * 32, jb = blockIdx.y * 32;
  for (int r = ty; r < 32; r += 8) {
    const int i = i0 + r, j = jb + tx;
    tile[r][tx] = (i < n && j < mc) ? X[(size_t)i * stride + j] : 0.0;
  }
  __syncthreads();
  for (int c = ty; c < 32; c += 8) {
    const int j = jb + c, i = i0 + tx;
    if (i < n && j < mc) {
      const double am = amax[j];
      const double sc = (am > 0.0 && am <= DBL_MAX) ? 1.0 / am : 1.0;
      Yout[(size_t)j * ldy + i] = tile[tx][c] * sc;
    }
  }
}

__device__ __forceinline__ double block_sum_256(double v, double* sh) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}

// unit 2-norm columns (entries are <= 1 in magnitude on entry: no overflow in the sum of squares)
__global__ __launch_bounds__(256) void col_normalize_kernel(double* __restrict__ Y, int ldy, int n) {
  __shared__ double sh[4];
  double* col = Y + (size_t)blockIdx.x * ldy;
  double ss = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) ss += col[i] * col[i];
  ss = block_sum_256(ss, sh);
  if (!(ss > 0.0) || !(ss <= DBL_MAX)) return;   // zero / non-finite column: the Cholesky factorisation refuses it
  const double sc = 1.0 / sqrt(ss);
  for (int i = threadIdx.x; i < n; i += 256) col[i] *= sc;
}

// TQ = T Q for the band matrix: TQ(i, j) = sum_off T(i, i + off) Q(i + off, j)
template <int B>
__global__ __launch_bounds__(256) void band_apply_kernel(int n, int m, int lde, const double* __restrict__ d,
                                                         const double* __restrict__ e, const double* __restrict__ Q, int ldq,
                                                         double* __restrict__ TQ, int ldt) {
  for (int j = blockIdx.y; j < m; j += gridDim.y) {   // the grid's y extent is capped: m may exceed it
    const double* q = Q + (size_t)j * ldq;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
      double v = d[i] * q[i];
#pragma unroll
      for (int b = 1; b <= B; ++b) {
        if (i - b >= 0) v += e[(size_t)(b - 1) * lde + i] * q[i - b];
        if (i + b < n) v += e[(size_t)(b - 1) * lde + i + b] * q[i + b];
      }
      TQ[(size_t)j * ldt + i] = v;
    }
  }
}

// ---- blocked Cholesky G = L L^T (lower triangle, in place) and X <- X L^-T ------------------------------------------
constexpr int CH_NB = 64;

// diagonal block [k0, k0 + nb): unblocked factorisation in LDS.  stat = {breakdown flag, min diag(L), max diag(L)}
__global__ __launch_bounds__(256) void chol_diag_kernel(double* __restrict__ G, int ldg, int k0, int nb, double* __restrict__ stat) {
  __shared__ double A[CH_NB][CH_NB + 1];
  __shared__ int bad;
  const int tid = threadIdx.x;
  if (tid == 0) bad = 0;
  for (int q = tid; q < nb * nb; q += 256) {
    const int i = q % nb, c = q / nb;
    A[i][c] = (i >= c) ? G[(size_t)(k0 + c) * ldg + k0 + i] : 0.0;
  }
  __syncthreads();
  for (int jj = 0; jj < nb; ++jj) {
    if (tid == 0) {
      const double v = A[jj][jj];
      if (!(v > 0.0) || !(v <= DBL_MAX)) { bad = 1; A[jj][jj] = 1.0; }
      else A[jj][jj] = sqrt(v);
    }
    __syncthreads();
    const double r = 1.0 / A[jj][jj];
    for (int i = jj + 1 + tid; i < nb; i += 256) A[i][jj] *= r;
    __syncthreads();
    const int rem = nb - jj - 1;
    for (int q = tid; q < rem * rem; q += 256) {
      const int i = jj + 1 + q % rem, c = jj + 1 + q / rem;
      if (i >= c) A[i][c] -= A[i][jj] * A[c][jj];
    }
    __syncthreads();
  }
  for (int q = tid; q < nb * nb; q += 256) {
    const int i = q % nb, c = q / nb;
    if (i >= c) G[(size_t)(k0 + c) * ldg + k0 + i] = A[i][c];
  }
  if (tid == 0) {
    double mn = stat[1], mx = stat[2];
    for (int jj = 0; jj < nb; ++jj) { mn = fmin(mn, A[jj][jj]); mx = fmax(mx, A[jj][jj]); }
    stat[1] = mn; stat[2] = mx;
    if (bad) stat[0] = 1.0;
  }
}

// rows [row0, row0 + nrows) of X, columns [k0, k0 + nb): x <- x L_kk^-T with L_kk the diagonal block of Lmat at k0.
// One thread per row (consecutive threads = consecutive rows of a column-major X: coalesced), L_kk in LDS.
__global__ __launch_bounds__(256) void trsm_rows_kernel(double* __restrict__ X, int ldx, int row0, int nrows, int k0, int nb,
                                                        const double* __restrict__ Lmat, int ldl) {
  __shared__ double Ls[CH_NB][CH_NB + 1];
  for (int q = threadIdx.x; q < nb * nb; q += 256) {
    const int i = q % nb, c = q / nb;
    Ls[i][c] = (i >= c) ? Lmat[(size_t)(k0 + c) * ldl + k0 + i] : 0.0;
  }
  __syncthreads();
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= nrows) return;
  double* x = X + (size_t)k0 * ldx + row0 + r;
  for (int c = 0; c < nb; ++c) {
    double v = x[(size_t)c * ldx];
    for (int t = 0; t < c; ++t) v -= x[(size_t)t * ldx] * Ls[c][t];
    x[(size_t)c * ldx] = v / Ls[c][c];
  }
}

__global__ void stat_init_kernel(double* stat) { stat[0] = 0.0; stat[1] = DBL_MAX; stat[2] = 0.0; }

// G (m x m, lower triangle significant) -> L in place; stat as in chol_diag_kernel
void cholesky_dev(hipStream_t st, int m, double* G, int ldg, double* stat) {
  hipLaunchKernelGGL(stat_init_kernel, dim3(1), dim3(1), 0, st, stat);
  for (int k0 = 0; k0 < m; k0 += CH_NB) {
    const int nb = std::min(CH_NB, m - k0), k1 = k0 + nb, rest = m - k1;
    hipLaunchKernelGGL(chol_diag_kernel, dim3(1), dim3(256), 0, st, G, ldg, k0, nb, stat);
    if (rest > 0) {
      hipLaunchKernelGGL(trsm_rows_kernel, dim3(ceil_div(rest, 256)), dim3(256), 0, st, G, ldg, k1, rest, k0, nb, (const double*)G, ldg);
      const double* Pn = G + (size_t)k0 * ldg + k1;
      dgemm_dev(st, 'N', 'T', rest, rest, nb, -1.0, Pn, ldg, Pn, ldg, 1.0, G + (size_t)k1 * ldg + k1, ldg);
    }
  }
}

// Y (n x m) <- Y L^-T, block column by block column
void trsm_right_dev(hipStream_t st, int n, int m, double* Y, int ldy, const double* L, int ldl) {
  for (int k0 = 0; k0 < m; k0 += CH_NB) {
    const int nb = std::min(CH_NB, m - k0), k1 = k0 + nb, rest = m - k1;
    hipLaunchKernelGGL(trsm_rows_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, Y, ldy, 0, n, k0, nb, L, ldl);
    if (rest > 0)
      dgemm_dev(st, 'N', 'T', n, rest, nb, -1.0, Y + (size_t)k0 * ldy, ldy, L + (size_t)k0 * ldl + k1, ldl, 1.0,
                Y + (size_t)k1 * ldy, ldy);
  }
}

}  // namespace

// key 17: percent 0 .. 100, or negative = automatic; key 18: 0 / 1; key 19: log10 of the bound, 0 .. 16.  A value
// outside that is refused (-1), like an unknown key
int set_range_knob(int key, int v) {
  int* p = key == 17 ? &g_range_pct : key == 18 ? &g_range_optin : key == 19 ? &g_range_logcond : nullptr;
  if (!p) return -1;
  if ((key == 17 && v > 100) || (key == 18 && v != 0 && v != 1) || (key == 19 && (v < 0 || v > 16))) return -1;
  const int old = *p;
  *p = (key == 17 && v < 0) ? -1 : v;
  return old;
}
int get_range_knob(int key) { return key == 17 ? g_range_pct : key == 18 ? g_range_optin : key == 19 ? g_range_logcond : -1; }
RangeInfo& range_info() { return g_range_info; }
// the size rule: does a window of m of n take the subset path?
bool range_takes_subset(int n, int m) {
  const int pct = g_range_pct >= 0 ? g_range_pct : range_auto_pct(n);
  return (long)100 * m <= (long)pct * n;
}

// m approximate eigenvalues w_sel of the band matrix (d, e) -> Ritz values w_out[m] (ascending) and an orthonormal n x m
// eigenvector basis z(ldz, m).  Returns EIGX_OK, or 1 (a Cholesky factorisation broke down) / 2 (cond(L) above the bound):
// z and w_out are then not to be used.  cond_out (optional) = the conditioning estimate.  Synchronous.
int band_eigvec_dev(Context& ctx, int n, int m, const double* d, const double* e, int lde, int band, const double* w_sel,
                    double* w_out, double* z, int ldz, double* cond_out, double* stage_s) {
  hipStream_t st = ctx.stream;
  if (cond_out) *cond_out = 0.0;
  double tbuf[2] = {0.0, 0.0};
  double* ts = stage_s ? stage_s : tbuf;   // seconds: [0] inverse iteration, [1] orthonormalisation + Rayleigh-Ritz
  const double t0 = now_s();

  // ---- host side: ||T|| (largest absolute row sum), sorted shifts nudged apart (DSTEIN) ---------------------------
  std::vector<double> hd((size_t)n), he((size_t)lde * band), hw((size_t)m);
  EIGX_HIP_CHECK(hipMemcpyAsync(hd.data(), d, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  EIGX_HIP_CHECK(hipMemcpyAsync(he.data(), e, (size_t)lde * band * 8, hipMemcpyDeviceToHost, st));
  EIGX_HIP_CHECK(hipMemcpyAsync(hw.data(), w_sel, (size_t)m * 8, hipMemcpyDeviceToHost, st));
  EIGX_HIP_CHECK(hipStreamSynchronize(st));
  double tnorm = 0.0;
  for (int i = 0; i < n; ++i) {
    double r = fabs(hd[i]);
    for (int b = 1; b <= band; ++b) {
      if (i - b >= 0) r += fabs(he[(size_t)(b - 1) * lde + i]);
      if (i + b < n) r += fabs(he[(size_t)(b - 1) * lde + i + b]);
    }
    tnorm = std::max(tnorm, r);
  }
  if (!(tnorm > 0.0)) tnorm = 1.0;   // zero matrix: any orthonormal basis will do
  const double eps_t = DBL_EPSILON * tnorm;
  std::sort(hw.begin(), hw.end());
  for (int j = 1; j < m; ++j)
    if (hw[j] - hw[j - 1] < 10.0 * eps_t) hw[j] = hw[j - 1] + 10.0 * eps_t;
  double* lam = ctx.pool.get_t<double>("sub.lam", (size_t)m);
  EIGX_HIP_CHECK(hipMemcpyAsync(lam, hw.data(), (size_t)m * 8, hipMemcpyHostToDevice, st));

  // ---- inverse iteration, a chunk of columns at a time ---------------------------------------------------------------
  const int ldy = pad_ld(n);
  double* Y = ctx.pool.get_t<double>("sub.Y", (size_t)ldy * m);
  const int per = (3 * band + 3) * 8 + 1;   // scratch bytes per matrix row and vector: U, L, X, Y + the pivot byte
  const double budget = std::min(4.0 * 1073741824.0, std::max((double)n * n * 8.0, 16.0 * 1048576.0));
  int mc_max = (int)(budget / ((double)n * per)) / 64 * 64;
  if (mc_max < 64) mc_max = 64;
  const int stride = std::min((m + 63) / 64 * 64, mc_max);
  IIArgs a;
  a.n = n; a.lde = lde; a.d = d; a.e = e; a.stride = stride; a.eps_t = eps_t;
  a.U = ctx.pool.get_t<double>("sub.U", (size_t)n * (2 * band + 1) * stride);
  a.L = ctx.pool.get_t<double>("sub.L", (size_t)n * band * stride);
  a.P = ctx.pool.get_t<unsigned char>("sub.P", (size_t)n * stride);
  a.X = ctx.pool.get_t<double>("sub.X", (size_t)n * stride);
  a.Y = ctx.pool.get_t<double>("sub.Yf", (size_t)n * stride);
  a.amax = ctx.pool.get_t<double>("sub.amax", (size_t)stride);
  for (int j0 = 0; j0 < m; j0 += stride) {
    a.mc = std::min(stride, m - j0); a.j0 = j0; a.lam = lam + j0;
    if (band == 1) hipLaunchKernelGGL(inviter_kernel<1>, dim3(ceil_div(a.mc, 64)), dim3(64), 0, st, a);
    else hipLaunchKernelGGL(inviter_kernel<2>, dim3(ceil_div(a.mc, 64)), dim3(64), 0, st, a);
    hipLaunchKernelGGL(ii_transpose_kernel, dim3(ceil_div(n, 32), ceil_div(a.mc, 32)), dim3(256), 0, st, (const double*)a.X,
                       (const double*)a.amax, n, a.mc, stride, Y + (size_t)j0 * ldy, ldy);
  }
  hipLaunchKernelGGL(col_normalize_kernel, dim3(m), dim3(256), 0, st, Y, ldy, n);
  EIGX_HIP_CHECK(hipStreamSynchronize(st));
  const double t1 = now_s();
  ts[0] = t1 - t0;

  // ---- CholQR2 -----------------------------------------------------------------------------------------------------------
  const int ldg = pad_ld(m + 2);
  double* G = ctx.pool.get_t<double>("sub.G", (size_t)ldg * m);
  double* stat = ctx.pool.get_t<double>("sub.stat", 8);
  double cond = 0.0;
  for (int pass = 0; pass < 2; ++pass) {
    dgemm_dev(st, 'T', 'N', m, m, n, 1.0, Y, ldy, Y, ldy, 0.0, G, ldg);
    cholesky_dev(st, m, G, ldg, stat);
    double hs[3];
    EIGX_HIP_CHECK(hipMemcpyAsync(hs, stat, sizeof(hs), hipMemcpyDeviceToHost, st));
    EIGX_HIP_CHECK(hipStreamSynchronize(st));
    if (pass == 0) {
      cond = (hs[0] == 0.0 && hs[1] > 0.0) ? hs[2] / hs[1] : std::numeric_limits<double>::infinity();
      if (cond_out) *cond_out = cond;
    }
    if (hs[0] != 0.0) { ts[1] = now_s() - t1; return 1; }
    if (pass == 0 && !(cond <= pow(10.0, (double)g_range_logcond))) { ts[1] = now_s() - t1; return 2; }
    trsm_right_dev(st, n, m, Y, ldy, G, ldg);
  }

  // ---- Rayleigh-Ritz: H = Q^T (T Q), H = S W S^T by the library's own full path, Z = Q S ---------------------------------
  const dim3 ga(std::min(ceil_div(n, 256), 64), std::min(m, 32768));
  if (band == 1) hipLaunchKernelGGL(band_apply_kernel<1>, ga, dim3(256), 0, st, n, m, lde, d, e, (const double*)Y, ldy, z, ldz);
  else hipLaunchKernelGGL(band_apply_kernel<2>, ga, dim3(256), 0, st, n, m, lde, d, e, (const double*)Y, ldy, z, ldz);
  double* H = G;   // the Gram matrix is no longer needed
  dgemm_dev(st, 'T', 'N', m, m, n, 1.0, Y, ldy, z, ldz, 0.0, H, ldg);
  // the inner solve has its own d / e and eigenvector buffer; red.* / dc.* / bt.* are free at this point (see the header)
  const int ldem = (m + 3) / 4 * 4;
  double* d2 = ctx.pool.get_t<double>("sub.hd", (size_t)m);
  double* e2 = ctx.pool.get_t<double>("sub.he", (size_t)ldem * 2);
  double* S = ctx.pool.get_t<double>("sub.S", (size_t)ldg * m);
  band_reduce_dev(ctx, m, H, ldg, d2, e2, ldem, 128, 2);
  EIGX_HIP_CHECK(hipStreamSynchronize(st));
  ctx.dc_zero_n = 0;
  band_dc_dev(ctx, m, m, d2, e2, ldem, 2, w_out, S, ldg);
  trbak_dev(ctx, m, m, H, ldg, S, ldg, e2, ldem, 128, 2);
  dgemm_dev(st, 'N', 'N', n, m, m, 1.0, Y, ldy, S, ldg, 0.0, z, ldz);
  EIGX_HIP_CHECK(hipStreamSynchronize(st));
  EIGX_HIP_CHECK(hipGetLastError());
  ts[1] = now_s() - t1;
  return EIGX_OK;
}

}  // namespace eigx

using namespace eigx;

extern "C" {

int eigx_band_bisect_range_dev(int n, int il, int iu, const double* d, const double* e, int lde, int band, double* w) {
  if (!g_ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  if (n <= 0 || il < 1 || iu > n || il > iu || lde < n || (band != 1 && band != 2) || !d || !e || !w) return EIGX_ERR_BAD_ARG;
  return eigx_guard(g_ctx, [&] {
    EIGX_HIP_CHECK(hipStreamSynchronize(nullptr));
    band_bisect_range_dev(g_ctx, n, il, iu, d, e, lde, band, w);
    return EIGX_OK;
  });
}

int eigx_band_eigvec_dev(int n, int m, const double* d, const double* e, int lde, int band, const double* w_sel, double* w_out,
                         double* z, int ldz) {
  if (!g_ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  if (n <= 0 || m < 1 || m > n || lde < n || (band != 1 && band != 2) || !d || !e || !w_sel || !w_out || !z || ldz < n)
    return EIGX_ERR_BAD_ARG;
  if (g_ctx.grid.nranks != 1) return EIGX_ERR_BAD_ARG;
  return eigx_guard(g_ctx, [&] {
    EIGX_HIP_CHECK(hipStreamSynchronize(nullptr));
    return band_eigvec_dev(g_ctx, n, m, d, e, lde, band, w_sel, w_out, z, ldz, nullptr, nullptr);
  });
}

int eigx_range_info(int* path, int* m, double* cond) {
  const RangeInfo& r = range_info();
  if (path) *path = r.path;
  if (m) *m = r.m;
  if (cond) *cond = r.cond;
  return EIGX_OK;
}

int eigx_range_timers(double* out4) {
  if (!out4) return EIGX_ERR_BAD_ARG;
  for (int q = 0; q < 4; ++q) out4[q] = range_info().t[q];
  return EIGX_OK;
}

}  // extern "C"
