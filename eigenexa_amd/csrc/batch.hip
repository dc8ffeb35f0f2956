// batch.hip -- eigx_s_batch (EXTENSION, not in the reference): many small symmetric eigenproblems (n <= EIGX_BATCH_NMAX) in one
// launch, one workgroup per matrix, the matrix resident in LDS from load to store.
//   load the upper triangle, mirror it, scan for NaN / Inf, scale (the rule of eigen_scaling, solver.hip)
//   -> Householder tridiagonalisation in the shape of EISPACK's tred2, Q accumulated in place
//   -> implicit QL with Wilkinson shift (EISPACK tql2 / LAPACK dsteqr): one lane computes the rotations of a QL iteration
//      into LDS, then every row's thread applies the whole sequence to its row of Q and tests the e[m] for deflation
//   -> sort ascending, unscale, store w(1:n), z(1:n, 1:n).
// No workgroup talks to another: no grid-wide barrier, no spin-wait, no atomics on the data.  Every sum is taken in an order
// that depends on n alone, so a matrix's result does not depend on its position in the batch or on the batch size.
// Matrices larger than the cutoff (eigx_tune key 21) go through solve_dev (eigen_s) one by one.
#include "eigx_context.h"
#include "batch_common.h"
#include "../../include/eigenexa_amd.h"
#include <algorithm>
#include <cfloat>
#include <limits>

// a*b + c is written out as fma() where it is wanted: the rank-2 update of the reduction has to round A(j, k) and A(k, j) alike
#pragma clang fp contract(off)

namespace eigx {
namespace {

int g_batch_nmax = EIGX_BATCH_NMAX;   // key 21: largest n served by the batch kernel

// One workgroup of 2 NMAX threads per matrix (NMAX = 32, 64, 96, 128: the n-classes): thread (r, hh) = (row, half).  The full symmetric matrix, then Q, lives in
// A(LD, NMAX), column-major with LD = NMAX + 1: row-wise loops (lane = row, a fixed column) are stride-1 across lanes, and
// the one column-wise loop (lane = column) has a stride of LD doubles = 2 banks mod 64.  Where a loop runs over columns the
// two halves share it; the application of the QL rotations is a chain along a row and uses the threads of half 0 only.
template <int NMAX>
__global__ __launch_bounds__(2 * NMAX) void batch_kernel(int n, int batch, const double* __restrict__ a, int lda, int64_t stride_a,
                                                         double* __restrict__ w, int ldw, double* __restrict__ z, int ldz,
                                                         int64_t stride_z, int want_vec, int* __restrict__ info,
                                                         unsigned long long* __restrict__ first) {
  constexpr int NT = 2 * NMAX, LD = NMAX + 1;
  __shared__ double A[LD * NMAX];
  __shared__ double d[NMAX], e[NMAX], hv[NMAX], u[NMAX], q[NMAX];
  __shared__ double pt[2 * NMAX];        // the two halves' partial sums; (c_i, s_i) of a QL iteration
  __shared__ double red[4][4];           // wave partials of block_sum / block_max
  __shared__ int perm[NMAX];
  __shared__ int ctl[4];                 // QL: top index m, lowest rotation, state
  __shared__ unsigned long long msk[2];  // QL: bit m = e[m] is negligible
  const int tid = threadIdx.x, r = tid % NMAX, hh = tid / NMAX;
  const bool row = hh == 0 && r < n;     // the thread that owns row r where one thread per row is wanted

  for (int k = blockIdx.x; k < batch; k += gridDim.x) {
    // ---- 1. load the upper triangle, mirror, scan, scale -------------------------------------------------------------------
    const double* ak = a + (size_t)k * stride_a;
    double mx = 0.0, bad = 0.0;
    for (int j = hh; j < n; j += 2) {
      if (r <= j) {
        const double x = ak[r + (size_t)j * lda];
        if (!(fabs(x) <= DBL_MAX)) bad = 1.0;
        else mx = fmax(mx, fabs(x));
        A[r + j * LD] = x;
        A[j + r * LD] = x;
      }
    }
    bad = block_max<NT>(bad, red[0]);
    mx = block_max<NT>(mx, red[1]);      // (its barrier also publishes the mirrored entries)
    if (bad != 0.0) {                    // uniform
      if (row) w[(size_t)k * ldw + r] = std::numeric_limits<double>::quiet_NaN();
      if (tid == 0) report_failure(first, info, k, EIGX_ERR_NONFINITE);
      __syncthreads();
      continue;
    }
    // outside [1e-90, 1e90]: scale by the power of two nearest to 1 / max|a| (eigen_scaling, solver.hip)
    double unscale = 1.0;
    if (mx > 0.0 && (mx < 1e-90 || mx > 1e90)) {
      int ex = 0;
      (void)frexp(mx, &ex);
      ex = ex < -1000 ? -1000 : ex;      // (a denormal max|a|: 2^-ex has to stay finite)
      const double sigma = ldexp(1.0, -ex);
      unscale = ldexp(1.0, ex);
      if (r < n)
        for (int j = hh; j < n; j += 2) A[r + j * LD] *= sigma;
    }
    if (row) perm[r] = r;
    __syncthreads();

    // ---- 2., 3. tridiagonalisation, Q in place, implicit QL (batch_common.h) -------------------------------------------------
    if (sym_tridiag_ql<NMAX>(n, want_vec, A, d, e, hv, u, q, pt, red, ctl, msk) == ST_FAIL) {   // uniform
      if (row) w[(size_t)k * ldw + r] = std::numeric_limits<double>::quiet_NaN();
      if (tid == 0) report_failure(first, info, k, EIGX_ERR_INTERNAL);
      __syncthreads();
      continue;
    }

    // ---- 4. sort ascending (rank by counting, ties by index), unscale, store -------------------------------------------------
    if (row) {
      const int rank = ascending_rank(n, d, r);
      perm[rank] = r;
      w[(size_t)k * ldw + rank] = d[r] * unscale;
    }
    if (tid == 0 && info) info[k] = 0;
    __syncthreads();
    if (want_vec && r < n) {
      double* zk = z + (size_t)k * stride_z;
      for (int j = hh; j < n; j += 2) zk[r + (size_t)j * ldz] = A[r + perm[j] * LD];
    }
    __syncthreads();
  }
}

}  // namespace

// kind: host <-> device copy of `batch` blocks of n x n doubles; one call where both sides are evenly spaced columns
void copy_blocks(double* dst, int ldd, int64_t sd, const double* src, int lds, int64_t ss, int n, int b0, int nb, hipMemcpyKind kind) {
  if (nb <= 0) return;
  if (sd == (int64_t)ldd * n && ss == (int64_t)lds * n) {
    EIGX_HIP_CHECK(hipMemcpy2D(dst + (size_t)b0 * sd, (size_t)ldd * 8, src + (size_t)b0 * ss, (size_t)lds * 8, (size_t)n * 8,
                               (size_t)n * nb, kind));
    return;
  }
  for (int k = b0; k < b0 + nb; ++k)
    EIGX_HIP_CHECK(hipMemcpy2D(dst + (size_t)k * sd, (size_t)ldd * 8, src + (size_t)k * ss, (size_t)lds * 8, (size_t)n * 8, (size_t)n, kind));
}

namespace {

// what both entry points require of their arguments (mode in upper case)
bool batch_args_ok(int n, int batch, const double* a, int lda, int64_t stride_a, const double* w, int ldw, const double* z, int ldz,
                   int64_t stride_z, char mode) {
  if (n < 1 || batch < 0 || lda < n || ldw < n || (mode != 'A' && mode != 'N')) return false;
  if (batch > 1 && stride_a < (int64_t)lda * n) return false;
  if (mode == 'A' && (ldz < n || (batch > 1 && stride_z < (int64_t)ldz * n))) return false;
  if (batch > 0 && (!a || !w || (mode == 'A' && !z))) return false;
  return true;
}

}  // namespace

int set_batch_nmax(int v) {
  if (v < 0 || v > EIGX_BATCH_NMAX) return -1;
  const int old = g_batch_nmax;
  g_batch_nmax = v;
  return old;
}

// device arrays; info_dev may be null
int batch_solve_dev(Context& ctx, int n, int batch, double* a, int lda, int64_t stride_a, double* w, int ldw, double* z, int ldz,
                    int64_t stride_z, char mode, int* info_dev) {
  if (!ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  if (ctx.grid.nranks != 1) return refuse_several_ranks(ctx);
  mode = upper_case(mode);
  if (!batch_args_ok(n, batch, a, lda, stride_a, w, ldw, z, ldz, stride_z, mode)) return EIGX_ERR_BAD_ARG;
  if (batch == 0) return EIGX_OK;
  EIGX_HIP_CHECK(hipSetDevice(ctx.device));
  EIGX_HIP_CHECK(hipStreamSynchronize(nullptr));   // the caller's default-stream work on the arguments (SolveFrame::begin)
  const double t0 = now_s();
  ctx.errinfo = 0;
  hipStream_t st = ctx.stream;
  const bool want_vec = mode == 'A';
  int rc = EIGX_OK;
  if (n > g_batch_nmax) {
    // above the cutoff: eigen_s with the interface's default block sizes, matrix by matrix
    for (int k = 0; k < batch; ++k) {
      const int rk = solve_dev(ctx, n, n, a + (size_t)k * stride_a, lda, w + (size_t)k * ldw, want_vec ? z + (size_t)k * stride_z : nullptr,
                               ldz, 48, 128, mode, 1, 1);
      if (rk != EIGX_OK && rk != EIGX_ERR_NONFINITE && rk != EIGX_ERR_INTERNAL) return rk;   // nothing per matrix: out of memory, ...
      if (info_dev) EIGX_HIP_CHECK(hipMemcpy(info_dev + k, &rk, sizeof(int), hipMemcpyHostToDevice));
      if (rc == EIGX_OK) rc = rk;
    }
  } else {
    unsigned long long* first = ctx.pool.get_t<unsigned long long>("batch.first", 1);
    EIGX_HIP_CHECK(hipMemsetAsync(first, 0xff, sizeof(unsigned long long), st));
    const dim3 grid((unsigned)batch);
    if (n <= 32)
      hipLaunchKernelGGL(batch_kernel<32>, grid, dim3(64), 0, st, n, batch, (const double*)a, lda, stride_a, w, ldw, z, ldz, stride_z,
                         (int)want_vec, info_dev, first);
    else if (n <= 64)
      hipLaunchKernelGGL(batch_kernel<64>, grid, dim3(128), 0, st, n, batch, (const double*)a, lda, stride_a, w, ldw, z, ldz, stride_z,
                         (int)want_vec, info_dev, first);
    else if (n <= 96)
      hipLaunchKernelGGL(batch_kernel<96>, grid, dim3(192), 0, st, n, batch, (const double*)a, lda, stride_a, w, ldw, z, ldz, stride_z,
                         (int)want_vec, info_dev, first);
    else
      hipLaunchKernelGGL(batch_kernel<128>, grid, dim3(256), 0, st, n, batch, (const double*)a, lda, stride_a, w, ldw, z, ldz, stride_z,
                         (int)want_vec, info_dev, first);
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

// Host arrays: a, z and w are staged in the pool buffers of the other host forms (host.a / host.z / host.w, leading dimension
// host_ld(n)), the per-matrix status words in batch.info.  w comes back for every matrix, z for those that succeeded.
static int batch_solve_host(Context& ctx, int n, int batch, double* a, int lda, int64_t stride_a, double* w, int ldw, double* z, int ldz,
                            int64_t stride_z, char mode, int* info) {
  if (!ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  if (ctx.grid.nranks != 1) return refuse_several_ranks(ctx);
  mode = upper_case(mode);
  if (!batch_args_ok(n, batch, a, lda, stride_a, w, ldw, z, ldz, stride_z, mode)) return EIGX_ERR_BAD_ARG;
  if (batch == 0) return EIGX_OK;
  EIGX_HIP_CHECK(hipSetDevice(ctx.device));
  const bool want_vec = mode == 'A';
  const int ldd = host_ld(n);
  const int64_t sd = (int64_t)ldd * n;
  double* ad = ctx.pool.get_t<double>("host.a", (size_t)sd * batch);
  double* zd = want_vec ? ctx.pool.get_t<double>("host.z", (size_t)sd * batch) : nullptr;
  double* wd = ctx.pool.get_t<double>("host.w", (size_t)n * batch);
  int* id = ctx.pool.get_t<int>("batch.info", (size_t)batch);
  copy_blocks(ad, ldd, sd, a, lda, batch > 1 ? stride_a : (int64_t)lda * n, n, 0, batch, hipMemcpyHostToDevice);
  const int rc = batch_solve_dev(ctx, n, batch, ad, ldd, sd, wd, n, zd, ldd, sd, mode, id);
  if (rc != EIGX_OK && rc != EIGX_ERR_NONFINITE && rc != EIGX_ERR_INTERNAL) return rc;
  std::vector<int> ih((size_t)batch);
  EIGX_HIP_CHECK(hipMemcpy(ih.data(), id, (size_t)batch * sizeof(int), hipMemcpyDeviceToHost));
  EIGX_HIP_CHECK(hipMemcpy2D(w, (size_t)ldw * 8, wd, (size_t)n * 8, (size_t)n * 8, (size_t)batch, hipMemcpyDeviceToHost));
  if (want_vec) {
    const int64_t sz = batch > 1 ? stride_z : (int64_t)ldz * n;
    for (int k = 0; k < batch;) {        // runs of matrices that succeeded
      int k1 = k;
      while (k1 < batch && ih[k1] == EIGX_OK) ++k1;
      copy_blocks(z, ldz, sz, zd, ldd, sd, n, k, k1 - k, hipMemcpyDeviceToHost);
      k = k1 + 1;
    }
  }
  if (info) std::copy(ih.begin(), ih.end(), info);
  return rc;
}

}  // namespace eigx

using namespace eigx;

extern "C" {

// EXTENSION: `batch` symmetric eigenproblems of one size (one GPU); see batch_solve_dev
int eigx_s_batch(int n, int batch, double* a, int lda, int64_t stride_a, double* w, int ldw, double* z, int ldz, int64_t stride_z,
                 char mode, int* info) {
  return eigx_guard(g_ctx, [&] { return batch_solve_host(g_ctx, n, batch, a, lda, stride_a, w, ldw, z, ldz, stride_z, mode, info); });
}
int eigx_s_batch_dev(int n, int batch, double* a_dev, int lda, int64_t stride_a, double* w_dev, int ldw, double* z_dev, int ldz,
                     int64_t stride_z, char mode, int* info_dev) {
  return eigx_guard(g_ctx, [&] {
    return batch_solve_dev(g_ctx, n, batch, a_dev, lda, stride_a, w_dev, ldw, z_dev, ldz, stride_z, mode, info_dev);
  });
}

}  // extern "C"
