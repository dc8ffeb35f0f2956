// hvbatch.hip -- eigx_h_vbatch (EXTENSION, not in the reference): a ragged batch of small complex Hermitian eigenproblems, the
// complex sibling of vbatch.hip: every block with its own order n[k], leading dimensions and offsets (in complex
// elements) into one interleaved buffer each for a and z and one real buffer for w.  The blocks at or below the cutoff (eigx_tune
// key 22, that of eigx_h_batch) are solved by one launch per non-empty n-class, one workgroup per block: the phases of
// hbatch_kernel (hbatch.hip) with n, the pointers and the leading dimensions taken from the workgroup's descriptor; the reduction,
// the phase chain and the QL iteration are herm_tridiag_ql of batch_common.h, so a block's w and z are bit for bit those of
// eigx_h_batch_dev(n, 1, ...).  No workgroup talks to another.  Blocks above the cutoff go through herm_solve_dev (eigen_h) one by
// one.  The schedule, the checks, the launches' failure word and the host staging are the frame of vbatch.hip.
#include "eigx_context.h"
#include "batch_common.h"
#include "../../include/eigenexa_amd.h"
#include <cfloat>

// (batch_common.h switches contraction off: the scaling and the unscaling are single products)
#pragma clang fp contract(off)

namespace eigx {
namespace {

// One workgroup of 2 NMAX threads per descriptor: thread (r, hh) = (row, half); LDS and access patterns are hbatch_kernel's.
// The descriptor's offsets of a and z count doubles.
template <int NMAX>
__global__ __launch_bounds__(2 * NMAX) void hvbatch_kernel(const VbDesc* __restrict__ desc, const double* __restrict__ a,
                                                           double* __restrict__ w, double* __restrict__ z, int want_vec,
                                                           int* __restrict__ info, unsigned long long* __restrict__ first) {
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
  const VbDesc ds = desc[blockIdx.x];    // uniform
  const int n = ds.n, k = ds.k, lda = ds.lda, ldz = ds.ldz;
  const int tid = threadIdx.x, r = tid % NMAX, hh = tid / NMAX;
  const bool row = hh == 0 && r < n;     // the thread that owns row r where one thread per row is wanted
  const double* ak = a + ds.off_a;
  double* wk = w + ds.off_w;

  // ---- 1. load the upper triangle, mirror with conjugation, scan, scale -------------------------------------------------------
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
      for (int j = hh; j < n; j += 2) { Ar[r + j * LD] *= sigma; Ai[r + j * LD] *= sigma; }
  }
  if (row) perm[r] = r;
  __syncthreads();

  // ---- 2., 3. tridiagonalisation, phase chain, Q D in place, implicit QL (batch_common.h) ---------------------------------------
  if (herm_tridiag_ql<NMAX>(n, want_vec, Ar, Ai, d, e, hv, pr, pi, ur, ui, qr, qi, pt, red, ctl, msk) == ST_FAIL) {   // uniform
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
    for (int j = hh; j < n; j += 2) {
      const int c = perm[j];
      const size_t at = 2 * (r + (size_t)j * ldz);
      zk[at] = Ar[r + c * LD];
      zk[at + 1] = Ai[r + c * LD];
    }
  }
}

void hvbatch_launch(int nclass, int count, const VbDesc* desc, const VbArgs& g, hipStream_t st, unsigned long long* first) {
  with_n_class<EIGX_HBATCH_NMAX>(nclass, [&](auto nmax) {
    constexpr int NMAX = decltype(nmax)::value;
    hipLaunchKernelGGL(hvbatch_kernel<NMAX>, dim3((unsigned)count), dim3(2 * NMAX), 0, st, desc, (const double*)g.a, g.w, g.z,
                       (int)(g.mode == 'A'), g.info, first);
  });
}
// above the cutoff: eigen_h with the interface's default block sizes (hbatch_solve_one, hbatch.hip)
int hvbatch_solve_one(Context& ctx, const VbArgs& g, int k) {
  const int n = g.n[k];
  return herm_solve_dev(ctx, n, n, g.block(g.a, g.off_a[k]), g.lda[k], g.w + g.off_w[k],
                        g.mode == 'A' ? g.block(g.z, g.off_z[k]) : nullptr, g.ldz ? g.ldz[k] : n, 48, 128, g.mode);
}

}  // namespace
}  // namespace eigx

using namespace eigx;

extern "C" {

// EXTENSION: `batch` complex Hermitian eigenproblems of their own sizes (one GPU; a, z interleaved complex; offsets and leading
// dimensions in complex elements); see vbatch_frame_host / vbatch_frame_dev (batch_frame.hip)
int eigx_h_vbatch(int batch, const int* n, double* a, const int64_t* off_a, const int* lda, double* w, const int64_t* off_w, double* z,
                  const int64_t* off_z, const int* ldz, char mode, int* info) {
  const VbArgs g{batch, n, a, off_a, lda, w, off_w, z, off_z, ldz, mode, info, 16};
  return eigx_guard(g_ctx, [&] { return vbatch_frame_host(g_ctx, g, get_hbatch_nmax(), EIGX_HBATCH_NMAX, hvbatch_launch, hvbatch_solve_one); });
}
int eigx_h_vbatch_dev(int batch, const int* n, double* a_dev, const int64_t* off_a, const int* lda, double* w_dev, const int64_t* off_w,
                      double* z_dev, const int64_t* off_z, const int* ldz, char mode, int* info_dev) {
  const VbArgs g{batch, n, a_dev, off_a, lda, w_dev, off_w, z_dev, off_z, ldz, mode, info_dev, 16};
  return eigx_guard(g_ctx, [&] { return vbatch_frame_dev(g_ctx, g, get_hbatch_nmax(), EIGX_HBATCH_NMAX, hvbatch_launch, hvbatch_solve_one); });
}

}  // extern "C"
