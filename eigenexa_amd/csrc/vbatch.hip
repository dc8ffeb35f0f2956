// vbatch.hip -- eigx_s_vbatch (EXTENSION, not in the reference): a ragged batch of small symmetric eigenproblems, every block with
// its own order n[k], leading dimensions and offsets into one buffer each for a, w and z.  The blocks at or
// below the cutoff (eigx_tune key 21, that of eigx_s_batch) are sorted by n-class on the host (eigx_vbatch_plan) and solved by one
// launch per non-empty class, one workgroup per block, the block resident in LDS from load to store: the phases of batch_kernel
// (batch.hip) with n, the pointers and the leading dimensions taken from the workgroup's descriptor; the reduction and the QL
// iteration are sym_tridiag_ql of batch_common.h, so a block's w and z are bit for bit those of eigx_s_batch_dev(n, 1, ...).
// No workgroup talks to another: no grid-wide barrier, no spin-wait, no atomics on the data.
// Blocks above the cutoff go through solve_dev (eigen_s) one by one; empty blocks (n = 0) are skipped.
// Here: the kernel and the two functions the frame of the ragged families asks for (vbatch_frame_dev / vbatch_frame_host with the
// schedule vbatch_plan, batch_frame.hip): the launch of one n-class and the full-size solve of one block.
#include "eigx_context.h"
#include "batch_common.h"
#include "../../include/eigenexa_amd.h"
#include <algorithm>
#include <cfloat>
#include <cstdlib>
#include <vector>

// (batch_common.h switches contraction off: the scaling and the unscaling are single products)
#pragma clang fp contract(off)

namespace eigx {
namespace {

// One workgroup of 2 NMAX threads per descriptor: thread (r, hh) = (row, half); LDS and access patterns are batch_kernel's.
template <int NMAX>
__global__ __launch_bounds__(2 * NMAX) void vbatch_kernel(const VbDesc* __restrict__ desc, const double* __restrict__ a,
                                                          double* __restrict__ w, double* __restrict__ z, int want_vec,
                                                          int* __restrict__ info, unsigned long long* __restrict__ first) {
  constexpr int NT = 2 * NMAX, LD = NMAX + 1;
  __shared__ double A[LD * NMAX];
  __shared__ double d[NMAX], e[NMAX], hv[NMAX], u[NMAX], q[NMAX];
  __shared__ double pt[2 * NMAX];        // the two halves' partial sums; (c_i, s_i) of a QL iteration
  __shared__ double red[4][4];           // wave partials of block_sum / block_max
  __shared__ int perm[NMAX];
  __shared__ int ctl[4];                 // QL: top index m, lowest rotation, state
  __shared__ unsigned long long msk[2];  // QL: bit m = e[m] is negligible
  const VbDesc ds = desc[blockIdx.x];    // uniform
  const int n = ds.n, k = ds.k, lda = ds.lda, ldz = ds.ldz;
  const int tid = threadIdx.x, r = tid % NMAX, hh = tid / NMAX;
  const bool row = hh == 0 && r < n;     // the thread that owns row r where one thread per row is wanted
  const double* ak = a + ds.off_a;
  double* wk = w + ds.off_w;

  // ---- 1. load the upper triangle, mirror, scan, scale -----------------------------------------------------------------------
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
  mx = block_max<NT>(mx, red[1]);        // (its barrier also publishes the mirrored entries)
  if (bad != 0.0) {                      // uniform
    if (row) wk[r] = std::numeric_limits<double>::quiet_NaN();
    if (tid == 0) report_failure(first, info, k, EIGX_ERR_NONFINITE);
    return;
  }
  // outside [1e-90, 1e90]: scale by the power of two nearest to 1 / max|a| (eigen_scaling, solver.hip)
  double unscale = 1.0;
  if (mx > 0.0 && (mx < 1e-90 || mx > 1e90)) {
    int ex = 0;
    (void)frexp(mx, &ex);
    ex = ex < -1000 ? -1000 : ex;        // (a denormal max|a|: 2^-ex has to stay finite)
    const double sigma = ldexp(1.0, -ex);
    unscale = ldexp(1.0, ex);
    if (r < n)
      for (int j = hh; j < n; j += 2) A[r + j * LD] *= sigma;
  }
  if (row) perm[r] = r;
  __syncthreads();

  // ---- 2., 3. tridiagonalisation, Q in place, implicit QL (batch_common.h) -----------------------------------------------------
  if (sym_tridiag_ql<NMAX>(n, want_vec, A, d, e, hv, u, q, pt, red, ctl, msk) == ST_FAIL) {   // uniform
    if (row) wk[r] = std::numeric_limits<double>::quiet_NaN();
    if (tid == 0) report_failure(first, info, k, EIGX_ERR_INTERNAL);
    return;
  }

  // ---- 4. sort ascending (rank by counting, ties by index), unscale, store -----------------------------------------------------
  if (row) {
    const int rank = ascending_rank(n, d, r);
    perm[rank] = r;
    wk[rank] = d[r] * unscale;
  }
  if (tid == 0 && info) info[k] = 0;
  __syncthreads();
  if (want_vec && r < n) {
    double* zk = z + ds.off_z;
    for (int j = hh; j < n; j += 2) zk[r + (size_t)j * ldz] = A[r + perm[j] * LD];
  }
}

void vbatch_launch(int nclass, int count, const VbDesc* desc, const VbArgs& g, hipStream_t st, unsigned long long* first) {
  with_n_class<EIGX_BATCH_NMAX>(nclass, [&](auto nmax) {
    constexpr int NMAX = decltype(nmax)::value;
    hipLaunchKernelGGL(vbatch_kernel<NMAX>, dim3((unsigned)count), dim3(2 * NMAX), 0, st, desc, (const double*)g.a, g.w, g.z,
                       (int)(g.mode == 'A'), g.info, first);
  });
}
// above the cutoff: eigen_s with the interface's default block sizes (batch_solve_one, batch.hip)
int vbatch_solve_one(Context& ctx, const VbArgs& g, int k) {
  const int n = g.n[k];
  return solve_dev(ctx, n, n, g.a + g.off_a[k], g.lda[k], g.w + g.off_w[k], g.mode == 'A' ? g.z + g.off_z[k] : nullptr,
                   g.ldz ? g.ldz[k] : n, 48, 128, g.mode, 1, 1);
}

}  // namespace

}  // namespace eigx

using namespace eigx;

extern "C" {

// EXTENSION: the schedule of a ragged batch (pure host arithmetic; works before eigx_init and without a GPU)
int eigx_vbatch_plan(int batch, const int* n, int cutoff, int top, int* order, int* counts6) {
  return vbatch_plan(batch, n, cutoff, top, order, counts6);
}

// EXTENSION: `batch` symmetric eigenproblems of their own sizes (one GPU); see vbatch_frame_host / vbatch_frame_dev
int eigx_s_vbatch(int batch, const int* n, double* a, const int64_t* off_a, const int* lda, double* w, const int64_t* off_w, double* z,
                  const int64_t* off_z, const int* ldz, char mode, int* info) {
  const VbArgs g{batch, n, a, off_a, lda, w, off_w, z, off_z, ldz, mode, info, 8};
  return eigx_guard(g_ctx, [&] { return vbatch_frame_host(g_ctx, g, get_batch_nmax(), EIGX_BATCH_NMAX, vbatch_launch, vbatch_solve_one); });
}
int eigx_s_vbatch_dev(int batch, const int* n, double* a_dev, const int64_t* off_a, const int* lda, double* w_dev, const int64_t* off_w,
                      double* z_dev, const int64_t* off_z, const int* ldz, char mode, int* info_dev) {
  const VbArgs g{batch, n, a_dev, off_a, lda, w_dev, off_w, z_dev, off_z, ldz, mode, info_dev, 8};
  return eigx_guard(g_ctx, [&] { return vbatch_frame_dev(g_ctx, g, get_batch_nmax(), EIGX_BATCH_NMAX, vbatch_launch, vbatch_solve_one); });
}

}  // extern "C"
