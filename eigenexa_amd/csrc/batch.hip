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
// Here: the kernel, the cutoff and the two functions the frame of the batch families asks for (batch_frame_dev / batch_frame_host,
// batch_frame.hip): the launch by n-class and the full-size solve of one matrix.  The kernels of the families share batch_common.h.
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
