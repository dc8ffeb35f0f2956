// gvbatch.hip -- eigx_gev_vbatch (EXTENSION, not in the reference): a ragged batch of small symmetric-definite pencils
// A x = lambda B x, every block with its own order n[k], leading dimensions and offsets into one buffer each for a, b, w and z
// (DESIGN section 8m).  The blocks at or below the cutoff (eigx_tune key 23, that of eigx_gev_batch) are sorted by n-class on the
// host (eigx_vbatch_plan) and solved by one launch per non-empty class, one workgroup per block, both matrices resident in LDS
// from load to store: the phases of gbatch_kernel (gbatch.hip) with n, the offsets and the leading dimensions taken from the
// workgroup's descriptor; the substitutions are solve_ut / solve_u of batch_solve.h, the reduction and the QL iteration are
// sym_tridiag_ql of batch_common.h, so a block's w, z and U are bit for bit those of eigx_gev_batch_dev(n, 1, ...).
// No workgroup talks to another: no grid-wide barrier, no spin-wait, no atomics on the data.  Every sum is taken in an order
// that depends on n alone.  Blocks above the cutoff go through gbatch_solve_one (gev_range_dev) one by one; empty blocks are
// skipped.  The schedule, the checks, the launches' failure word and the host staging are the frame of vbatch.hip.
#include "eigx_context.h"
#include "batch_common.h"
#include "batch_solve.h"
#include "../../include/eigenexa_amd.h"
#include <algorithm>
#include <cfloat>

// (batch_common.h switches contraction off: every a*b + c that is wanted fused is written as fma())
#pragma clang fp contract(off)

namespace eigx {
namespace {

// One workgroup of 2 NMAX threads per descriptor: thread (r, hh) = (row, half); LDS and access patterns are gbatch_kernel's:
// S(LD, NMAX) holds A, then C, then Q, then Z; U(LD, NMAX) holds B, then its factor (upper triangle).
template <int NMAX>
__global__ __launch_bounds__(2 * NMAX) void gvbatch_kernel(const VbPencilDesc* __restrict__ desc, const double* __restrict__ a,
                                                           double* __restrict__ b, double* __restrict__ w, double* __restrict__ z,
                                                           int want_vec, int* __restrict__ info,
                                                           unsigned long long* __restrict__ first) {
  constexpr int NT = 2 * NMAX, LD = NMAX + 1;
  __shared__ double S[LD * NMAX];
  __shared__ double U[LD * NMAX];
  __shared__ double d[NMAX], e[NMAX], hv[NMAX], u[NMAX], q[NMAX];
  __shared__ double pt[2 * NMAX];        // the two halves' partial sums; (c_i, s_i) of a QL iteration
  __shared__ double red[4][4];           // wave partials of block_sum / block_max
  __shared__ int perm[NMAX];
  __shared__ int ctl[4];                 // QL: top index m, lowest rotation, state
  __shared__ unsigned long long msk[2];  // QL: bit m = e[m] is negligible
  const VbPencilDesc ds = desc[blockIdx.x];   // uniform
  const int n = ds.n, k = ds.k, lda = ds.lda, ldb = ds.ldb, ldz = ds.ldz;
  const int tid = threadIdx.x, r = tid % NMAX, hh = tid / NMAX;
  const bool row = hh == 0 && r < n;     // the thread that owns row r (or column r) where one thread per row is wanted
  const double* ak = a + ds.off_a;
  double* bk = b + ds.off_b;
  double* wk = w + ds.off_w;

  // ---- 1. load both upper triangles, mirror A, scan, scale -------------------------------------------------------------------
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
  mxb = block_max<NT>(mxb, red[2]);      // (the barriers also publish the loaded entries)
  if (bad != 0.0) return fail_block(k, EIGX_ERR_NONFINITE, row, r, wk, info, first);   // uniform
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

  // ---- 2. B = U^T U, right-looking: two barriers per column ------------------------------------------------------------------
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
  if (!spd) return fail_block(k, EIGX_ERR_NOT_SPD, row, r, wk, info, first);

  // ---- 3. C = U^-T A U^-1: X = U^-T A down the columns (lane = column), C = X U^-1 along the rows (lane = row) ------------------
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
  // (uniform: B was too close to singular for C to be formed)
  if (bad != 0.0) return fail_block(k, EIGX_ERR_NOT_SPD, row, r, wk, info, first);
  const int exc = scale_exponent(mxc, false);
  if (exc != 0 && r < n) {
    const double sigma = ldexp(1.0, -exc);
    for (int j = hh; j < n; j += 2) S[r + j * LD] *= sigma;
  }
  __syncthreads();

  // ---- 4. tridiagonalisation, Q in place, implicit QL (batch_common.h), sort --------------------------------------------------
  if (sym_tridiag_ql<NMAX>(n, want_vec, S, d, e, hv, u, q, pt, red, ctl, msk) == ST_FAIL)   // uniform
    return fail_block(k, EIGX_ERR_INTERNAL, row, r, wk, info, first);
  if (row) {
    const int rank = ascending_rank(n, d, r);
    perm[rank] = r;
    wk[rank] = ldexp(d[r], exa - exb + exc);   // C = 2^(exb - exa - exc) times the matrix that was solved
  }
  if (tid == 0 && info) info[k] = 0;

  // ---- 5. Z = U^-1 Y down the columns (lane = column), unscale, store -----------------------------------------------------------
  if (want_vec && row) solve_u<LD>(n, U, S + r * LD);
  __syncthreads();
  if (r < n) {
    if (want_vec) {
      double* zk = z + ds.off_z;
      for (int j = hh; j < n; j += 2) zk[r + (size_t)j * ldz] = ldexp(S[r + perm[j] * LD], -(exb / 2));
    }
    for (int j = hh; j < n; j += 2)
      if (r <= j) bk[r + (size_t)j * ldb] = ldexp(U[r + j * LD], exb / 2);
  }
}

void gvbatch_launch(int nclass, int count, const VbPencilDesc* desc, const VbArgs& g, hipStream_t st, unsigned long long* first) {
  with_n_class<EIGX_GBATCH_NMAX>(nclass, [&](auto nmax) {
    constexpr int NMAX = decltype(nmax)::value;
    hipLaunchKernelGGL(gvbatch_kernel<NMAX>, dim3((unsigned)count), dim3(2 * NMAX), 0, st, desc, (const double*)g.a, g.b, g.w, g.z,
                       (int)(g.mode == 'A'), g.info, first);
  });
}
// above the cutoff: block k as a uniform batch of one pencil through gbatch_solve_one (gbatch.hip)
int gvbatch_solve_one(Context& ctx, const VbArgs& g, int k) {
  const int n = g.n[k];
  const bool want_vec = g.mode == 'A';
  const BatchArgs one{n, 1, g.a + g.off_a[k], g.lda[k], 0, g.b + g.off_b[k], g.ldb[k], 0, g.w + g.off_w[k], n,
                      want_vec ? g.z + g.off_z[k] : nullptr, want_vec ? g.ldz[k] : n, 0, g.mode, nullptr, 8, true};
  return gbatch_solve_one(ctx, one, 0);
}

VbArgs gvbatch_args(int batch, const int* n, double* a, const int64_t* off_a, const int* lda, double* b, const int64_t* off_b,
                    const int* ldb, double* w, const int64_t* off_w, double* z, const int64_t* off_z, const int* ldz, char mode,
                    int* info) {
  VbArgs g{batch, n, a, off_a, lda, w, off_w, z, off_z, ldz, mode, info, 8};
  g.has_b = true;
  g.b = b;
  g.off_b = off_b;
  g.ldb = ldb;
  return g;
}

}  // namespace
}  // namespace eigx

using namespace eigx;

extern "C" {

// EXTENSION: `batch` symmetric-definite pencils of their own sizes (one GPU); see vbatch_frame_host / vbatch_frame_dev (batch_frame.hip)
int eigx_gev_vbatch(int batch, const int* n, double* a, const int64_t* off_a, const int* lda, double* b, const int64_t* off_b,
                    const int* ldb, double* w, const int64_t* off_w, double* z, const int64_t* off_z, const int* ldz, char mode,
                    int* info) {
  const VbArgs g = gvbatch_args(batch, n, a, off_a, lda, b, off_b, ldb, w, off_w, z, off_z, ldz, mode, info);
  return eigx_guard(g_ctx, [&] {
    return vbatch_frame_host(g_ctx, g, get_gbatch_nmax(), EIGX_GBATCH_NMAX, (VbPencilLaunch)gvbatch_launch, gvbatch_solve_one);
  });
}
int eigx_gev_vbatch_dev(int batch, const int* n, double* a_dev, const int64_t* off_a, const int* lda, double* b_dev,
                        const int64_t* off_b, const int* ldb, double* w_dev, const int64_t* off_w, double* z_dev, const int64_t* off_z,
                        const int* ldz, char mode, int* info_dev) {
  const VbArgs g = gvbatch_args(batch, n, a_dev, off_a, lda, b_dev, off_b, ldb, w_dev, off_w, z_dev, off_z, ldz, mode, info_dev);
  return eigx_guard(g_ctx, [&] {
    return vbatch_frame_dev(g_ctx, g, get_gbatch_nmax(), EIGX_GBATCH_NMAX, (VbPencilLaunch)gvbatch_launch, gvbatch_solve_one);
  });
}

}  // extern "C"
