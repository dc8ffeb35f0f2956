// hbatch.hip -- eigx_h_batch (EXTENSION, not in the reference): many small complex Hermitian eigenproblems (n <= EIGX_HBATCH_NMAX)
// in one launch, one workgroup per matrix, the matrix resident in LDS from load to store.  The complex
// sibling of batch.hip, the same kernel shape:
//   load the upper triangle (interleaved complex; of the diagonal the real parts only), mirror it with conjugation into the
//   split planes Ar, Ai, scan for NaN / Inf, scale by the rule of eigen_scaling
//   -> Householder tridiagonalisation in the shape of EISPACK's tred2 with Hermitian reflectors H = I - u u^H / h,
//      u = x - g e_l, g = -(x_l / |x_l|) ||x|| (the form of EISPACK's htridi, not LAPACK's zlarfg with a complex tau): the
//      tridiagonal matrix comes out Hermitian with the complex off-diagonal entries g
//   -> a chain of unit phases D (p_0 = 1, t = conj(p_{k-1}) g_k, e_k = |t|, p_k = conj(t) / |t|) makes D^H T D real with
//      e >= 0; Q = H_{n-1} ... H_1 is accumulated in place with p_k in place of the 1 of column k, which gives Q D
//   -> implicit QL with Wilkinson shift on the real (d, e), the sweep of batch.hip; the rotations are real, half 0 applies
//      them to the real plane of its row of Q and half 1 to the imaginary plane
//   -> sort ascending, unscale, store w(1:n), z(1:n, 1:n) interleaved.
// No workgroup talks to another: no grid-wide barrier, no spin-wait, no atomics on the data.  Every sum is taken in an order
// that depends on n alone, so a matrix's result does not depend on its position in the batch or on the batch size.
// Matrices larger than the cutoff (eigx_tune key 22) go through herm_solve_dev (eigen_h) one by one.
// Here: the kernel, the cutoff and the two functions the frame of the batch families asks for (batch_frame_dev / batch_frame_host,
// batch.hip: checks, launch and failure word, the loop above the cutoff, host staging); the reduction, the phase chain, the
// accumulation of Q D and the QL rounds are herm_tridiag_ql of batch_common.h, which hgbatch.hip calls too.
#include "eigx_context.h"
#include "batch_common.h"
#include "../../include/eigenexa_amd.h"
#include <cfloat>

// (batch_common.h switches contraction off: the rank-2 update has to round A(r, c) and conj(A(c, r)) alike)
#pragma clang fp contract(off)

namespace eigx {
namespace {

// One workgroup of 2 NMAX threads per matrix (NMAX = 32, 64, 96: the n-classes): thread (r, hh) = (row, half).  The full
// Hermitian matrix, then Q, lives in the planes Ar(LD, NMAX), Ai(LD, NMAX), column-major with LD = NMAX + 1: the access
// patterns are those of batch_kernel, once per plane.  Where a loop runs over columns the two halves share it; in the
// application of the QL rotations, a chain along a row, half 0 takes the real plane and half 1 the imaginary one.
template <int NMAX>
__global__ __launch_bounds__(2 * NMAX) void hbatch_kernel(int n, int batch, const double* __restrict__ a, int lda, int64_t stride_a,
                                                          double* __restrict__ w, int ldw, double* __restrict__ z, int ldz,
                                                          int64_t stride_z, int want_vec, int* __restrict__ info,
                                                          unsigned long long* __restrict__ first) {
  constexpr int NT = 2 * NMAX, LD = NMAX + 1;
  __shared__ double Ar[LD * NMAX], Ai[LD * NMAX];
  __shared__ double d[NMAX], e[NMAX], hv[NMAX];
  __shared__ double pr[NMAX], pi[NMAX];  // the off-diagonal entries g of the Hermitian tridiagonal matrix, then the phases
  __shared__ double ur[NMAX], ui[NMAX], qr[NMAX], qi[NMAX];
  __shared__ double pt[4 * NMAX];        // the two halves' partial sums (re, im); (c_i, s_i) of a QL iteration
  __shared__ double red[4][4];           // wave partials of block_sum / block_max
  __shared__ int perm[NMAX];
  __shared__ int ctl[4];                 // QL: top index m, lowest rotation, state
  __shared__ unsigned long long msk[2];  // QL: bit m = e[m] is negligible
  const int tid = threadIdx.x, r = tid % NMAX, hh = tid / NMAX;
  const bool row = hh == 0 && r < n;     // the thread that owns row r where one thread per row is wanted

  for (int k = blockIdx.x; k < batch; k += gridDim.x) {
    // ---- 1. load the upper triangle, mirror with conjugation, scan, scale ---------------------------------------------------
    const double* ak = a + 2 * (size_t)k * stride_a;
    double mx = 0.0, bad = 0.0;
    for (int j = hh; j < n; j += 2) {
      if (r <= j) {
        const size_t at = 2 * (r + (size_t)j * lda);
        const double xr = ak[at];
        const double xi = r < j ? ak[at + 1] : 0.0;   // the imaginary part of the diagonal is not read
        if (!(fabs(xr) <= DBL_MAX) || !(fabs(xi) <= DBL_MAX)) bad = 1.0;
        else mx = fmax(mx, fmax(fabs(xr), fabs(xi)));
        Ar[r + j * LD] = xr;
        Ai[r + j * LD] = xi;
        Ar[j + r * LD] = xr;
        Ai[j + r * LD] = -xi;
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
        for (int j = hh; j < n; j += 2) { Ar[r + j * LD] *= sigma; Ai[r + j * LD] *= sigma; }
    }
    if (row) perm[r] = r;
    __syncthreads();

    // ---- 2., 3. tridiagonalisation, phase chain, Q D in place, implicit QL (batch_common.h) -------------------------------------
    if (herm_tridiag_ql<NMAX>(n, want_vec, Ar, Ai, d, e, hv, pr, pi, ur, ui, qr, qi, pt, red, ctl, msk) == ST_FAIL) {   // uniform
      fail_matrix(k, EIGX_ERR_INTERNAL, row, r, w, ldw, info, first);
      continue;
    }

    // ---- 4. sort ascending (rank by counting, ties by index), unscale, store -------------------------------------------------
    if (row) {
      const double dr = d[r];
      int rank = 0;
      for (int j = 0; j < n; ++j) {
        const double dj = d[j];
        rank += (dj < dr || (dj == dr && j < r)) ? 1 : 0;
      }
      perm[rank] = r;
      w[(size_t)k * ldw + rank] = dr * unscale;
    }
    if (tid == 0 && info) info[k] = 0;
    __syncthreads();
    if (want_vec && r < n) {
      double* zk = z + 2 * (size_t)k * stride_z;
      for (int j = hh; j < n; j += 2) {
        const int c = perm[j];
        const size_t at = 2 * (r + (size_t)j * ldz);
        zk[at] = Ar[r + c * LD];
        zk[at + 1] = Ai[r + c * LD];
      }
    }
    __syncthreads();
  }
}

int g_hbatch_nmax = EIGX_HBATCH_NMAX;   // key 22: largest n served by the batch kernel

void hbatch_launch(const BatchArgs& g, hipStream_t st, unsigned long long* first) {
  with_n_class<EIGX_HBATCH_NMAX>(g.n, [&](auto nmax) {
    constexpr int NMAX = decltype(nmax)::value;
    hipLaunchKernelGGL(hbatch_kernel<NMAX>, dim3((unsigned)g.batch), dim3(2 * NMAX), 0, st, g.n, g.batch, (const double*)g.a, g.lda,
                       g.stride_a, g.w, g.ldw, g.z, g.ldz, g.stride_z, (int)(g.mode == 'A'), g.info, first);
  });
}
// above the cutoff: eigen_h with the interface's default block sizes
int hbatch_solve_one(Context& ctx, const BatchArgs& g, int k) {
  return herm_solve_dev(ctx, g.n, g.n, g.block(g.a, g.stride_a, k), g.lda, g.w + (size_t)k * g.ldw,
                        g.mode == 'A' ? g.block(g.z, g.stride_z, k) : nullptr, g.ldz, 48, 128, g.mode);
}

}  // namespace

int set_hbatch_nmax(int v) {
  if (v < 0 || v > EIGX_HBATCH_NMAX) return -1;
  const int old = g_hbatch_nmax;
  g_hbatch_nmax = v;
  return old;
}
int get_hbatch_nmax() { return g_hbatch_nmax; }

}  // namespace eigx

using namespace eigx;

extern "C" {

// EXTENSION: `batch` complex Hermitian eigenproblems of one size (one GPU; a, z interleaved complex; lda, ldz and the strides in
// complex elements); see batch_frame_host / batch_frame_dev (batch_frame.hip)
int eigx_h_batch(int n, int batch, double* a, int lda, int64_t stride_a, double* w, int ldw, double* z, int ldz, int64_t stride_z,
                 char mode, int* info) {
  const BatchArgs g{n, batch, a, lda, stride_a, nullptr, 0, 0, w, ldw, z, ldz, stride_z, mode, info, 16, false};
  return eigx_guard(g_ctx, [&] { return batch_frame_host(g_ctx, g, g_hbatch_nmax, hbatch_launch, hbatch_solve_one); });
}
int eigx_h_batch_dev(int n, int batch, double* a_dev, int lda, int64_t stride_a, double* w_dev, int ldw, double* z_dev, int ldz,
                     int64_t stride_z, char mode, int* info_dev) {
  const BatchArgs g{n, batch, a_dev, lda, stride_a, nullptr, 0, 0, w_dev, ldw, z_dev, ldz, stride_z, mode, info_dev, 16, false};
  return eigx_guard(g_ctx, [&] { return batch_frame_dev(g_ctx, g, g_hbatch_nmax, hbatch_launch, hbatch_solve_one); });
}

}  // extern "C"
