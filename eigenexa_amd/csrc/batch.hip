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
// This file also holds the host side of all three batch families (eigx_h_batch: hbatch.hip, eigx_gev_batch: gbatch.hip): the
// argument check, the device entry (batch_frame_dev: prologue, the loop above the cutoff, the launch and its first-failure
// word, the timers), the host entry (batch_frame_host: staging in the pool, copy in, copy back) and copy_blocks.  A family
// supplies its kernel launch by n-class and its full-size solve of one matrix; the kernels share batch_common.h.
#include "eigx_context.h"
#include "batch_common.h"
#include "../../include/eigenexa_amd.h"
#include <algorithm>
#include <cfloat>

// a*b + c is written out as fma() where it is wanted: the rank-2 update of the reduction has to round A(j, k) and A(k, j) alike
#pragma clang fp contract(off)

namespace eigx {
namespace {

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
      fail_matrix(k, EIGX_ERR_NONFINITE, row, r, w, ldw, info, first);
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
      fail_matrix(k, EIGX_ERR_INTERNAL, row, r, w, ldw, info, first);
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

int g_batch_nmax = EIGX_BATCH_NMAX;   // key 21: largest n served by the batch kernel

void batch_launch(const BatchArgs& g, hipStream_t st, unsigned long long* first) {
  with_n_class<EIGX_BATCH_NMAX>(g.n, [&](auto nmax) {
    constexpr int NMAX = decltype(nmax)::value;
    hipLaunchKernelGGL(batch_kernel<NMAX>, dim3((unsigned)g.batch), dim3(2 * NMAX), 0, st, g.n, g.batch, (const double*)g.a, g.lda,
                       g.stride_a, g.w, g.ldw, g.z, g.ldz, g.stride_z, (int)(g.mode == 'A'), g.info, first);
  });
}
// above the cutoff: eigen_s with the interface's default block sizes
int batch_solve_one(Context& ctx, const BatchArgs& g, int k) {
  return solve_dev(ctx, g.n, g.n, g.block(g.a, g.stride_a, k), g.lda, g.w + (size_t)k * g.ldw,
                   g.mode == 'A' ? g.block(g.z, g.stride_z, k) : nullptr, g.ldz, 48, 128, g.mode, 1, 1);
}

}  // namespace

int set_batch_nmax(int v) {
  if (v < 0 || v > EIGX_BATCH_NMAX) return -1;
  const int old = g_batch_nmax;
  g_batch_nmax = v;
  return old;
}
int get_batch_nmax() { return g_batch_nmax; }

// ---- the frame of the three families (declared in eigx_context.h) ------------------------------------------------------------
bool batch_status_per_matrix(int rc) {   // (solve_dev and herm_solve_dev never return EIGX_ERR_NOT_SPD: one set serves all)
  return rc == EIGX_OK || rc == EIGX_ERR_NONFINITE || rc == EIGX_ERR_NOT_SPD || rc == EIGX_ERR_INTERNAL;
}

void copy_blocks(void* dst, int ldd, int64_t sd, const void* src, int lds, int64_t ss, int n, int b0, int nb, int esz, hipMemcpyKind kind) {
  if (nb <= 0) return;
  char* d = (char*)dst;
  const char* s = (const char*)src;
  const size_t e = (size_t)esz;
  if (sd == (int64_t)ldd * n && ss == (int64_t)lds * n) {
    EIGX_HIP_CHECK(hipMemcpy2D(d + e * b0 * sd, e * ldd, s + e * b0 * ss, e * lds, e * n, (size_t)n * nb, kind));
    return;
  }
  for (int k = b0; k < b0 + nb; ++k) EIGX_HIP_CHECK(hipMemcpy2D(d + e * k * sd, e * ldd, s + e * k * ss, e * lds, e * n, (size_t)n, kind));
}

// what both entries require of their arguments (mode in upper case)
static bool batch_args_ok(const BatchArgs& g) {
  const int n = g.n, batch = g.batch;
  if (n < 1 || batch < 0 || g.lda < n || g.ldw < n || (g.mode != 'A' && g.mode != 'N')) return false;
  if (batch > 1 && g.stride_a < (int64_t)g.lda * n) return false;
  if (g.has_b && (g.ldb < n || (batch > 1 && g.stride_b < (int64_t)g.ldb * n))) return false;
  if (g.mode == 'A' && (g.ldz < n || (batch > 1 && g.stride_z < (int64_t)g.ldz * n))) return false;
  if (batch > 0 && (!g.a || (g.has_b && !g.b) || !g.w || (g.mode == 'A' && !g.z))) return false;
  return true;
}
// What both entries begin with.  Returns true to go on (g.mode in upper case, the device set), or false with the status to
// return in rc: a refusal, or EIGX_OK for an empty batch.
static bool batch_begin(Context& ctx, BatchArgs& g, int& rc) {
  rc = EIGX_OK;
  if (!ctx.initialized) {
    rc = EIGX_ERR_NOT_INITIALIZED;
    return false;
  }
  if (ctx.grid.nranks != 1) {
    rc = refuse_several_ranks(ctx);
    return false;
  }
  g.mode = upper_case(g.mode);
  if (!batch_args_ok(g)) {
    rc = EIGX_ERR_BAD_ARG;
    return false;
  }
  if (g.batch == 0) return false;
  EIGX_HIP_CHECK(hipSetDevice(ctx.device));
  return true;
}

int batch_frame_dev(Context& ctx, BatchArgs g, int cutoff, BatchLaunch launch, BatchSolveOne solve_one) {
  int rc;
  if (!batch_begin(ctx, g, rc)) return rc;
  EIGX_HIP_CHECK(hipStreamSynchronize(nullptr));   // the caller's default-stream work on the arguments (SolveFrame::begin)
  const double t0 = now_s();
  ctx.errinfo = 0;
  hipStream_t st = ctx.stream;
  if (g.n > cutoff) {
    // above the cutoff: the full-size solver, matrix by matrix; the first failure is the call's status
    for (int k = 0; k < g.batch; ++k) {
      const int rk = solve_one(ctx, g, k);
      if (!batch_status_per_matrix(rk)) return rk;   // nothing per matrix: out of memory, ...
      if (g.info) EIGX_HIP_CHECK(hipMemcpy(g.info + k, &rk, sizeof(int), hipMemcpyHostToDevice));
      if (rc == EIGX_OK) rc = rk;
    }
  } else {
    unsigned long long* first = ctx.pool.get_t<unsigned long long>("batch.first", 1);
    // memset 0xff of the first-failure word: all ones = "no matrix failed"; a failed one leaves (index << 8 | -code) by atomicMin
    EIGX_HIP_CHECK(hipMemsetAsync(first, 0xff, sizeof(unsigned long long), st));
    launch(g, st, first);
    EIGX_HIP_CHECK(hipGetLastError());
    unsigned long long f = 0;
    EIGX_HIP_CHECK(hipMemcpyAsync(&f, first, sizeof(f), hipMemcpyDeviceToHost, st));
    EIGX_HIP_CHECK(hipStreamSynchronize(st));
    if (f != ~0ull) {                    // (index << 8 | -code) of the first matrix that failed
      rc = -(int)(f & 0xff);
      ctx.errinfo = -1;
    }
  }
  for (int q = 0; q < 16; ++q) ctx.timers[q] = 0.0;
  ctx.timers[0] = now_s() - t0;
  return rc;
}

// Host arrays: a, b, z and w are staged in the pool buffers of the other host forms (host.a / host.b / host.z, or host.ha / host.hz
// at 16 bytes per element, and host.w; leading dimension host_ld(n)), the per-matrix status words in batch.info.  info and w
// come back for every matrix; z (mode 'A') and b (U, every mode) for those that succeeded: a failed matrix's stay untouched.
int batch_frame_host(Context& ctx, BatchArgs g, int cutoff, BatchLaunch launch, BatchSolveOne solve_one) {
  int rc;
  if (!batch_begin(ctx, g, rc)) return rc;
  const int n = g.n, batch = g.batch, esz = g.esz, ldd = host_ld(n);
  const bool want_vec = g.mode == 'A', cplx = esz == 16;
  const int64_t sd = (int64_t)ldd * n;
  const size_t bytes = (size_t)esz * sd * batch;
  BatchArgs dv = g;                      // the same call on the staged arrays
  dv.a = (double*)ctx.pool.get(cplx ? "host.ha" : "host.a", bytes);
  dv.b = g.has_b ? (double*)ctx.pool.get(cplx ? "host.hb" : "host.b", bytes) : nullptr;
  dv.z = want_vec ? (double*)ctx.pool.get(cplx ? "host.hz" : "host.z", bytes) : nullptr;
  dv.w = ctx.pool.get_t<double>("host.w", (size_t)n * batch);
  dv.info = ctx.pool.get_t<int>("batch.info", (size_t)batch);
  dv.lda = dv.ldb = dv.ldz = ldd;
  dv.stride_a = dv.stride_b = dv.stride_z = sd;
  dv.ldw = n;
  const int64_t sa = batch > 1 ? g.stride_a : (int64_t)g.lda * n, sb = batch > 1 ? g.stride_b : (int64_t)g.ldb * n,
                sz = batch > 1 ? g.stride_z : (int64_t)g.ldz * n;
  copy_blocks(dv.a, ldd, sd, g.a, g.lda, sa, n, 0, batch, esz, hipMemcpyHostToDevice);
  if (g.has_b) copy_blocks(dv.b, ldd, sd, g.b, g.ldb, sb, n, 0, batch, esz, hipMemcpyHostToDevice);
  rc = batch_frame_dev(ctx, dv, cutoff, launch, solve_one);
  if (!batch_status_per_matrix(rc)) return rc;
  std::vector<int> ih((size_t)batch);
  EIGX_HIP_CHECK(hipMemcpy(ih.data(), dv.info, (size_t)batch * sizeof(int), hipMemcpyDeviceToHost));
  EIGX_HIP_CHECK(hipMemcpy2D(g.w, (size_t)g.ldw * 8, dv.w, (size_t)n * 8, (size_t)n * 8, (size_t)batch, hipMemcpyDeviceToHost));
  // z and b come back in runs of matrices that succeeded (one copy_blocks per run): what the caller holds for a failed one stays
  for (int k = 0; k < batch;) {
    int k1 = k;
    while (k1 < batch && ih[k1] == EIGX_OK) ++k1;
    if (want_vec) copy_blocks(g.z, g.ldz, sz, dv.z, ldd, sd, n, k, k1 - k, esz, hipMemcpyDeviceToHost);
    if (g.has_b) copy_blocks(g.b, g.ldb, sb, dv.b, ldd, sd, n, k, k1 - k, esz, hipMemcpyDeviceToHost);
    k = k1 + 1;
  }
  if (g.info) std::copy(ih.begin(), ih.end(), g.info);
  return rc;
}

}  // namespace eigx

using namespace eigx;

extern "C" {

// EXTENSION: `batch` symmetric eigenproblems of one size (one GPU); see batch_frame_host / batch_frame_dev
int eigx_s_batch(int n, int batch, double* a, int lda, int64_t stride_a, double* w, int ldw, double* z, int ldz, int64_t stride_z,
                 char mode, int* info) {
  const BatchArgs g{n, batch, a, lda, stride_a, nullptr, 0, 0, w, ldw, z, ldz, stride_z, mode, info, 8, false};
  return eigx_guard(g_ctx, [&] { return batch_frame_host(g_ctx, g, g_batch_nmax, batch_launch, batch_solve_one); });
}
int eigx_s_batch_dev(int n, int batch, double* a_dev, int lda, int64_t stride_a, double* w_dev, int ldw, double* z_dev, int ldz,
                     int64_t stride_z, char mode, int* info_dev) {
  const BatchArgs g{n, batch, a_dev, lda, stride_a, nullptr, 0, 0, w_dev, ldw, z_dev, ldz, stride_z, mode, info_dev, 8, false};
  return eigx_guard(g_ctx, [&] { return batch_frame_dev(g_ctx, g, g_batch_nmax, batch_launch, batch_solve_one); });
}

}  // extern "C"
