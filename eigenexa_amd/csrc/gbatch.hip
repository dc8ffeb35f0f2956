// gbatch.hip -- eigx_gev_batch (EXTENSION, not in the reference): many small symmetric-definite pencils A x = lambda B x
// (n <= EIGX_GBATCH_NMAX) in one launch, one workgroup per pencil, both matrices resident in LDS from load to store (DESIGN
// section 8j).  The Cholesky route of eigx_gev_range inside the kernel shape of batch.hip:
//   load the upper triangles of A (mirrored) and B, scan both for NaN / Inf, scale each by a power of two (B by an even one)
//   -> B = U^T U, upper and right-looking, one column per step
//   -> C = U^-T A U^-1: a forward substitution down every column, then the same along every row; mirrored, scanned, scaled
//   -> tridiagonalisation, Q in place, implicit QL: sym_tridiag_ql of batch_common.h, the code eigx_s_batch runs
//   -> sort ascending, Z = U^-1 Y by a backward substitution down every column, unscale, store w, z and U (into b).
// No workgroup talks to another: no grid-wide barrier, no spin-wait, no atomics on the data.  Every sum is taken in an order
// that depends on n alone, so a pencil's result does not depend on its position in the batch or on the batch size.
// Pencils larger than the cutoff (eigx_tune key 23) go through gev_range_dev (gev.hip) one by one.
#include "eigx_context.h"
#include "batch_common.h"
#include "../../include/eigenexa_amd.h"
#include <algorithm>
#include <cfloat>
#include <limits>

// (batch_common.h switches contraction off: every a*b + c that is wanted fused is written as fma())
#pragma clang fp contract(off)

namespace eigx {
namespace {

int g_gbatch_nmax = EIGX_GBATCH_NMAX;   // key 23: largest n served by the batch kernel

// the exponent ex of the scaling 2^-ex of a matrix whose largest entry is mx: 0 inside [1e-90, 1e90] (and for the zero
// matrix), else that of the power of two nearest to mx (the rule of batch_kernel); even: rounded up to an even number
__device__ inline int scale_exponent(double mx, bool even) {
  if (!(mx > 0.0 && (mx < 1e-90 || mx > 1e90))) return 0;
  int ex = 0;
  (void)frexp(mx, &ex);
  ex = ex < -1000 ? -1000 : ex;        // (a denormal maximum: 2^-ex has to stay finite)
  return even ? ex + (ex & 1) : ex;
}

// x(0 .. n-1), entry k at x[k * inc], <- U^-T x: x_k = (x_k - sum_{j < k} U(j, k) x_j) / U(k, k), k ascending.  The sum runs
// in four interleaved chains from +0: with U = I it is +0 and x_k comes back as it was, the sign of a zero included.
template <int LD>
__device__ inline void solve_ut(int n, const double* U, double* x, int inc) {
  for (int k = 0; k < n; ++k) {
    const double* uk = U + k * LD;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int j = 0;
    for (; j + 3 < k; j += 4) {
      s0 = fma(uk[j], x[j * inc], s0);
      s1 = fma(uk[j + 1], x[(j + 1) * inc], s1);
      s2 = fma(uk[j + 2], x[(j + 2) * inc], s2);
      s3 = fma(uk[j + 3], x[(j + 3) * inc], s3);
    }
    for (; j < k; ++j) s0 = fma(uk[j], x[j * inc], s0);
    x[k * inc] = (x[k * inc] - ((s0 + s1) + (s2 + s3))) / uk[k];
  }
}
// x(0 .. n-1) <- U^-1 x: x_k = (x_k - sum_{j > k} U(k, j) x_j) / U(k, k), k descending, the sums as above
template <int LD>
__device__ inline void solve_u(int n, const double* U, double* x) {
  for (int k = n - 1; k >= 0; --k) {
    const double* uk = U + k;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int j = k + 1;
    for (; j + 3 < n; j += 4) {
      s0 = fma(uk[j * LD], x[j], s0);
      s1 = fma(uk[(j + 1) * LD], x[j + 1], s1);
      s2 = fma(uk[(j + 2) * LD], x[j + 2], s2);
      s3 = fma(uk[(j + 3) * LD], x[j + 3], s3);
    }
    for (; j < n; ++j) s0 = fma(uk[j * LD], x[j], s0);
    x[k] = (x[k] - ((s0 + s1) + (s2 + s3))) / uk[k * LD];
  }
}

// One workgroup of 2 NMAX threads per pencil (NMAX = 32, 64, 96: the n-classes): thread (r, hh) = (row, half) as in
// batch_kernel.  S(LD, NMAX) holds A, then C, then Q, then Z; U(LD, NMAX) holds B, then its factor (upper triangle; the
// strict lower triangle is never read); column-major with LD = NMAX + 1, the access patterns of batch_kernel: lane = row at
// a fixed column is stride 1, lane = column is a stride of LD doubles, an entry of U that all lanes read is a broadcast.
template <int NMAX>
__global__ __launch_bounds__(2 * NMAX) void gbatch_kernel(int n, int batch, const double* __restrict__ a, int lda, int64_t stride_a,
                                                          double* __restrict__ b, int ldb, int64_t stride_b, double* __restrict__ w,
                                                          int ldw, double* __restrict__ z, int ldz, int64_t stride_z, int want_vec,
                                                          int* __restrict__ info, unsigned long long* __restrict__ first) {
  constexpr int NT = 2 * NMAX, LD = NMAX + 1;
  __shared__ double S[LD * NMAX];
  __shared__ double U[LD * NMAX];
  __shared__ double d[NMAX], e[NMAX], hv[NMAX], u[NMAX], q[NMAX];
  __shared__ double pt[2 * NMAX];        // the two halves' partial sums; (c_i, s_i) of a QL iteration
  __shared__ double red[4][4];           // wave partials of block_sum / block_max
  __shared__ int perm[NMAX];
  __shared__ int ctl[4];                 // QL: top index m, lowest rotation, state
  __shared__ unsigned long long msk[2];  // QL: bit m = e[m] is negligible
  const int tid = threadIdx.x, r = tid % NMAX, hh = tid / NMAX;
  const bool row = hh == 0 && r < n;     // the thread that owns row r (or column r) where one thread per row is wanted
  const double nan = std::numeric_limits<double>::quiet_NaN();

  for (int k = blockIdx.x; k < batch; k += gridDim.x) {
    // ---- 1. load both upper triangles, mirror A, scan, scale -----------------------------------------------------------------
    const double* ak = a + (size_t)k * stride_a;
    double* bk = b + (size_t)k * stride_b;
    double mxa = 0.0, mxb = 0.0, bad = 0.0;
    for (int j = hh; j < n; j += 2) {
      if (r <= j) {
        const double xa = ak[r + (size_t)j * lda], xb = bk[r + (size_t)j * ldb];
        if (!(fabs(xa) <= DBL_MAX) || !(fabs(xb) <= DBL_MAX)) bad = 1.0;
        else { mxa = fmax(mxa, fabs(xa)); mxb = fmax(mxb, fabs(xb)); }
        S[r + j * LD] = xa;
        S[j + r * LD] = xa;
        U[r + j * LD] = xb;
      }
    }
    bad = block_max<NT>(bad, red[0]);
    mxa = block_max<NT>(mxa, red[1]);
    mxb = block_max<NT>(mxb, red[2]);    // (the barriers also publish the loaded entries)
    if (bad != 0.0) {                    // uniform; b is as it was passed
      if (row) w[(size_t)k * ldw + r] = nan;
      if (tid == 0) report_failure(first, info, k, EIGX_ERR_NONFINITE);
      __syncthreads();
      continue;
    }
    // A by 2^-exa, B by 2^-exb with exb even: the factor of the caller's B is 2^(exb / 2) times the computed one
    const int exa = scale_exponent(mxa, false), exb = scale_exponent(mxb, true);
    if (exa != 0 && r < n) {
      const double sigma = ldexp(1.0, -exa);
      for (int j = hh; j < n; j += 2) S[r + j * LD] *= sigma;
    }
    if (exb != 0 && r < n) {
      const double sigma = ldexp(1.0, -exb);
      for (int j = hh; j < n; j += 2)
        if (r <= j) U[r + j * LD] *= sigma;
    }
    if (row) perm[r] = r;
    __syncthreads();

    // ---- 2. B = U^T U, right-looking: two barriers per column ----------------------------------------------------------------
    bool spd = true;
    for (int c = 0; c < n; ++c) {
      const double p = U[c + c * LD];
      if (!(p > 0.0) || !(p <= DBL_MAX)) {   // the rule of eigx_chol_dev (uniform)
        spd = false;
        break;
      }
      const double s = sqrt(p);
      if (row && r > c) U[c + r * LD] = U[c + r * LD] / s;
      __syncthreads();
      if (tid == 0) U[c + c * LD] = s;       // (every thread has read the pivot; nothing below reads the diagonal)
      if (r > c && r < n) {                  // the trailing block, lane = row: U(r, j) -= U(c, r) U(c, j), j >= r
        const double ur = U[c + r * LD];
        for (int j = c + 1 + hh; j < n; j += 2) {
          const double uj = U[c + j * LD], x = U[r + j * LD];
          if (r <= j) U[r + j * LD] = fma(-ur, uj, x);
        }
      }
      __syncthreads();
    }
    if (!spd) {
      if (row) w[(size_t)k * ldw + r] = nan;
      if (tid == 0) report_failure(first, info, k, EIGX_ERR_NOT_SPD);
      __syncthreads();
      continue;
    }

    // ---- 3. C = U^-T A U^-1: X = U^-T A down the columns (lane = column), C = X U^-1 along the rows (lane = row) ----------------
    if (row) solve_ut<LD>(n, U, S + r * LD, 1);
    __syncthreads();
    if (row) solve_ut<LD>(n, U, S + r, LD);
    __syncthreads();
    // the upper triangle over the lower one (the reduction wants C(r, c) and C(c, r) to be one number), scan, scale
    double mxc = 0.0;
    if (r < n) {
      for (int j = hh; j < n; j += 2) {
        if (r <= j) {
          const double x = S[r + j * LD];
          if (!(fabs(x) <= DBL_MAX)) bad = 1.0;
          else mxc = fmax(mxc, fabs(x));
          S[j + r * LD] = x;
        }
      }
    }
    bad = block_max<NT>(bad, red[0]);
    mxc = block_max<NT>(mxc, red[1]);
    if (bad != 0.0) {                    // uniform: B was too close to singular for C to be formed
      if (row) w[(size_t)k * ldw + r] = nan;
      if (tid == 0) report_failure(first, info, k, EIGX_ERR_NOT_SPD);
      __syncthreads();
      continue;
    }
    const int exc = scale_exponent(mxc, false);
    if (exc != 0 && r < n) {
      const double sigma = ldexp(1.0, -exc);
      for (int j = hh; j < n; j += 2) S[r + j * LD] *= sigma;
    }
    __syncthreads();

    // ---- 4. tridiagonalisation, Q in place, implicit QL (batch_common.h), sort ------------------------------------------------
    if (sym_tridiag_ql<NMAX>(n, want_vec, S, d, e, hv, u, q, pt, red, ctl, msk) == ST_FAIL) {   // uniform
      if (row) w[(size_t)k * ldw + r] = nan;
      if (tid == 0) report_failure(first, info, k, EIGX_ERR_INTERNAL);
      __syncthreads();
      continue;
    }
    if (row) {
      const int rank = ascending_rank(n, d, r);
      perm[rank] = r;
      w[(size_t)k * ldw + rank] = ldexp(d[r], exa - exb + exc);   // C = 2^(exb - exa - exc) times the matrix that was solved
    }
    if (tid == 0 && info) info[k] = 0;

    // ---- 5. Z = U^-1 Y down the columns (lane = column), unscale, store ---------------------------------------------------------
    if (want_vec && row) solve_u<LD>(n, U, S + r * LD);
    __syncthreads();
    if (r < n) {
      if (want_vec) {
        double* zk = z + (size_t)k * stride_z;
        for (int j = hh; j < n; j += 2) zk[r + (size_t)j * ldz] = ldexp(S[r + perm[j] * LD], -(exb / 2));
      }
      for (int j = hh; j < n; j += 2)
        if (r <= j) bk[r + (size_t)j * ldb] = ldexp(U[r + j * LD], exb / 2);
    }
    __syncthreads();
  }
}

// what both entry points require of their arguments (mode in upper case): the rules of eigx_s_batch, and the same for b
bool gbatch_args_ok(int n, int batch, const double* a, int lda, int64_t stride_a, const double* b, int ldb, int64_t stride_b,
                    const double* w, int ldw, const double* z, int ldz, int64_t stride_z, char mode) {
  if (n < 1 || batch < 0 || lda < n || ldb < n || ldw < n || (mode != 'A' && mode != 'N')) return false;
  if (batch > 1 && (stride_a < (int64_t)lda * n || stride_b < (int64_t)ldb * n)) return false;
  if (mode == 'A' && (ldz < n || (batch > 1 && stride_z < (int64_t)ldz * n))) return false;
  if (batch > 0 && (!a || !b || !w || (mode == 'A' && !z))) return false;
  return true;
}

bool per_pencil(int rc) { return rc == EIGX_OK || rc == EIGX_ERR_NONFINITE || rc == EIGX_ERR_NOT_SPD || rc == EIGX_ERR_INTERNAL; }

// Above the cutoff: gev_range_dev with il = 1, iu = n, pencil by pencil.  It wants even leading dimensions: a pencil with an odd
// lda, ldb or ldz is staged through the pool buffers gbatch.a / gbatch.b / gbatch.z, and U and z are copied out where it succeeded.
int gbatch_loop_dev(Context& ctx, int n, int batch, double* a, int lda, int64_t stride_a, double* b, int ldb, int64_t stride_b,
                    double* w, int ldw, double* z, int ldz, int64_t stride_z, char mode, int* info_dev) {
  const bool want_vec = mode == 'A';
  const bool stage = ((lda | ldb) & 1) || (want_vec && (ldz & 1));
  const int lds = pad_ld(n);
  const size_t col = (size_t)n * 8;
  double *as = nullptr, *bs = nullptr, *zs = nullptr;
  if (stage) {
    as = ctx.pool.get_t<double>("gbatch.a", (size_t)lds * n);
    bs = ctx.pool.get_t<double>("gbatch.b", (size_t)lds * n);
    if (want_vec) zs = ctx.pool.get_t<double>("gbatch.z", (size_t)lds * n);
  }
  int rc = EIGX_OK;
  for (int k = 0; k < batch; ++k) {
    double* ak = a + (size_t)k * stride_a;
    double* bk = b + (size_t)k * stride_b;
    double* zk = want_vec ? z + (size_t)k * stride_z : nullptr;
    int rk;
    if (stage) {
      EIGX_HIP_CHECK(hipMemcpy2D(as, (size_t)lds * 8, ak, (size_t)lda * 8, col, (size_t)n, hipMemcpyDeviceToDevice));
      EIGX_HIP_CHECK(hipMemcpy2D(bs, (size_t)lds * 8, bk, (size_t)ldb * 8, col, (size_t)n, hipMemcpyDeviceToDevice));
      rk = gev_range_dev(ctx, n, RangeWindow::index(1, n), as, lds, bs, lds, w + (size_t)k * ldw, zs, lds, mode);
      if (rk == EIGX_OK) {
        EIGX_HIP_CHECK(hipMemcpy2D(bk, (size_t)ldb * 8, bs, (size_t)lds * 8, col, (size_t)n, hipMemcpyDeviceToDevice));
        if (want_vec) EIGX_HIP_CHECK(hipMemcpy2D(zk, (size_t)ldz * 8, zs, (size_t)lds * 8, col, (size_t)n, hipMemcpyDeviceToDevice));
      }
    } else {
      rk = gev_range_dev(ctx, n, RangeWindow::index(1, n), ak, lda, bk, ldb, w + (size_t)k * ldw, zk, ldz, mode);
    }
    if (!per_pencil(rk)) return rk;      // nothing per pencil: out of memory, ...
    if (info_dev) EIGX_HIP_CHECK(hipMemcpy(info_dev + k, &rk, sizeof(int), hipMemcpyHostToDevice));
    if (rc == EIGX_OK) rc = rk;
  }
  return rc;
}

}  // namespace

int set_gbatch_nmax(int v) {
  if (v < 0 || v > EIGX_GBATCH_NMAX) return -1;
  const int old = g_gbatch_nmax;
  g_gbatch_nmax = v;
  return old;
}

// device arrays; info_dev may be null
static int gbatch_solve_dev(Context& ctx, int n, int batch, double* a, int lda, int64_t stride_a, double* b, int ldb, int64_t stride_b,
                            double* w, int ldw, double* z, int ldz, int64_t stride_z, char mode, int* info_dev) {
  if (!ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  if (ctx.grid.nranks != 1) return refuse_several_ranks(ctx);
  mode = upper_case(mode);
  if (!gbatch_args_ok(n, batch, a, lda, stride_a, b, ldb, stride_b, w, ldw, z, ldz, stride_z, mode)) return EIGX_ERR_BAD_ARG;
  if (batch == 0) return EIGX_OK;
  EIGX_HIP_CHECK(hipSetDevice(ctx.device));
  EIGX_HIP_CHECK(hipStreamSynchronize(nullptr));   // the caller's default-stream work on the arguments (SolveFrame::begin)
  const double t0 = now_s();
  ctx.errinfo = 0;
  hipStream_t st = ctx.stream;
  const bool want_vec = mode == 'A';
  int rc = EIGX_OK;
  if (n > g_gbatch_nmax) {
    rc = gbatch_loop_dev(ctx, n, batch, a, lda, stride_a, b, ldb, stride_b, w, ldw, z, ldz, stride_z, mode, info_dev);
    if (!per_pencil(rc)) return rc;
  } else {
    unsigned long long* first = ctx.pool.get_t<unsigned long long>("gbatch.first", 1);
    EIGX_HIP_CHECK(hipMemsetAsync(first, 0xff, sizeof(unsigned long long), st));
    const dim3 grid((unsigned)batch);
    if (n <= 32)
      hipLaunchKernelGGL(gbatch_kernel<32>, grid, dim3(64), 0, st, n, batch, (const double*)a, lda, stride_a, b, ldb, stride_b, w, ldw,
                         z, ldz, stride_z, (int)want_vec, info_dev, first);
    else if (n <= 64)
      hipLaunchKernelGGL(gbatch_kernel<64>, grid, dim3(128), 0, st, n, batch, (const double*)a, lda, stride_a, b, ldb, stride_b, w, ldw,
                         z, ldz, stride_z, (int)want_vec, info_dev, first);
    else
      hipLaunchKernelGGL(gbatch_kernel<96>, grid, dim3(192), 0, st, n, batch, (const double*)a, lda, stride_a, b, ldb, stride_b, w, ldw,
                         z, ldz, stride_z, (int)want_vec, info_dev, first);
    EIGX_HIP_CHECK(hipGetLastError());
    unsigned long long f = 0;
    EIGX_HIP_CHECK(hipMemcpyAsync(&f, first, sizeof(f), hipMemcpyDeviceToHost, st));
    EIGX_HIP_CHECK(hipStreamSynchronize(st));
    if (f != ~0ull) {
      rc = -(int)(f & 0xff);
      ctx.errinfo = -1;
    }
  }
  for (int q = 0; q < 16; ++q) ctx.timers[q] = 0.0;
  ctx.timers[0] = now_s() - t0;
  return rc;
}

// Host arrays: a, b, z and w are staged in the pool buffers of the other host forms (host.a / host.b / host.z / host.w, leading
// dimension host_ld(n)), the per-pencil status words in gbatch.info.  w comes back for every pencil, z and U for those that
// succeeded.
static int gbatch_solve_host(Context& ctx, int n, int batch, double* a, int lda, int64_t stride_a, double* b, int ldb, int64_t stride_b,
                             double* w, int ldw, double* z, int ldz, int64_t stride_z, char mode, int* info) {
  if (!ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  if (ctx.grid.nranks != 1) return refuse_several_ranks(ctx);
  mode = upper_case(mode);
  if (!gbatch_args_ok(n, batch, a, lda, stride_a, b, ldb, stride_b, w, ldw, z, ldz, stride_z, mode)) return EIGX_ERR_BAD_ARG;
  if (batch == 0) return EIGX_OK;
  EIGX_HIP_CHECK(hipSetDevice(ctx.device));
  const bool want_vec = mode == 'A';
  const int ldd = host_ld(n);
  const int64_t sd = (int64_t)ldd * n;
  double* ad = ctx.pool.get_t<double>("host.a", (size_t)sd * batch);
  double* bd = ctx.pool.get_t<double>("host.b", (size_t)sd * batch);
  double* zd = want_vec ? ctx.pool.get_t<double>("host.z", (size_t)sd * batch) : nullptr;
  double* wd = ctx.pool.get_t<double>("host.w", (size_t)n * batch);
  int* id = ctx.pool.get_t<int>("gbatch.info", (size_t)batch);
  const int64_t sb = batch > 1 ? stride_b : (int64_t)ldb * n;
  copy_blocks(ad, ldd, sd, a, lda, batch > 1 ? stride_a : (int64_t)lda * n, n, 0, batch, hipMemcpyHostToDevice);
  copy_blocks(bd, ldd, sd, b, ldb, sb, n, 0, batch, hipMemcpyHostToDevice);
  const int rc = gbatch_solve_dev(ctx, n, batch, ad, ldd, sd, bd, ldd, sd, wd, n, zd, ldd, sd, mode, id);
  if (!per_pencil(rc)) return rc;
  std::vector<int> ih((size_t)batch);
  EIGX_HIP_CHECK(hipMemcpy(ih.data(), id, (size_t)batch * sizeof(int), hipMemcpyDeviceToHost));
  EIGX_HIP_CHECK(hipMemcpy2D(w, (size_t)ldw * 8, wd, (size_t)n * 8, (size_t)n * 8, (size_t)batch, hipMemcpyDeviceToHost));
  const int64_t sz = batch > 1 ? stride_z : (int64_t)ldz * n;
  for (int k = 0; k < batch;) {          // runs of pencils that succeeded
    int k1 = k;
    while (k1 < batch && ih[k1] == EIGX_OK) ++k1;
    if (want_vec) copy_blocks(z, ldz, sz, zd, ldd, sd, n, k, k1 - k, hipMemcpyDeviceToHost);
    copy_blocks(b, ldb, sb, bd, ldd, sd, n, k, k1 - k, hipMemcpyDeviceToHost);
    k = k1 + 1;
  }
  if (info) std::copy(ih.begin(), ih.end(), info);
  return rc;
}

}  // namespace eigx

using namespace eigx;

extern "C" {

// EXTENSION: `batch` symmetric-definite pencils of one size (one GPU); see gbatch_solve_dev
int eigx_gev_batch(int n, int batch, double* a, int lda, int64_t stride_a, double* b, int ldb, int64_t stride_b, double* w, int ldw,
                   double* z, int ldz, int64_t stride_z, char mode, int* info) {
  return eigx_guard(g_ctx, [&] {
    return gbatch_solve_host(g_ctx, n, batch, a, lda, stride_a, b, ldb, stride_b, w, ldw, z, ldz, stride_z, mode, info);
  });
}
int eigx_gev_batch_dev(int n, int batch, double* a_dev, int lda, int64_t stride_a, double* b_dev, int ldb, int64_t stride_b,
                       double* w_dev, int ldw, double* z_dev, int ldz, int64_t stride_z, char mode, int* info_dev) {
  return eigx_guard(g_ctx, [&] {
    return gbatch_solve_dev(g_ctx, n, batch, a_dev, lda, stride_a, b_dev, ldb, stride_b, w_dev, ldw, z_dev, ldz, stride_z, mode,
                            info_dev);
  });
}

}  // extern "C"
