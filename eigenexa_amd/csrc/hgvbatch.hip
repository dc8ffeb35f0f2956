// hgvbatch.hip -- eigx_hgev_vbatch (EXTENSION, not in the reference): a ragged batch of small Hermitian-definite pencils
// A x = lambda B x, the complex sibling of gvbatch.hip: every block with its own order n[k], leading
// dimensions and offsets (in complex elements) into one interleaved buffer each for a, b and z and one real buffer for w.  The
// blocks at or below the cutoff (eigx_tune key 24, that of eigx_hgev_batch) are solved by one launch per non-empty n-class (32,
// 64), one workgroup per block, both matrices as split planes in LDS from load to store: the phases of hgbatch_kernel
// (hgbatch.hip) with n, the offsets and the leading dimensions taken from the workgroup's descriptor; the substitutions are
// zsolve_ut / zsolve_u of batch_solve.h, the reduction, the phase chain and the QL iteration are herm_tridiag_ql of
// batch_common.h, so a block's w, z and U are bit for bit those of eigx_hgev_batch_dev(n, 1, ...).  No workgroup talks to
// another.  Blocks above the cutoff go through hgbatch_solve_one (hgev_range_dev) one by one.  The schedule, the checks, the
// launches' failure word and the host staging are the frame of vbatch.hip.
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

// One workgroup of 2 NMAX threads per descriptor: thread (r, hh) = (row, half); LDS and access patterns are hgbatch_kernel's:
// the split planes Sr, Si(LD, NMAX) hold A, then C, then Q, then Z; Ur, Ui(LD, NMAX) hold B, then its factor (upper triangle).
// The descriptor's offsets of a, b and z count doubles.
template <int NMAX>
__global__ __launch_bounds__(2 * NMAX) void hgvbatch_kernel(const VbPencilDesc* __restrict__ desc, const double* __restrict__ a,
                                                            double* __restrict__ b, double* __restrict__ w, double* __restrict__ z,
                                                            int want_vec, int* __restrict__ info,
                                                            unsigned long long* __restrict__ first) {
  constexpr int NT = 2 * NMAX, LD = NMAX + 1;
  __shared__ double Sr[LD * NMAX], Si[LD * NMAX];
  __shared__ double Ur[LD * NMAX], Ui[LD * NMAX];
  __shared__ double d[NMAX], e[NMAX], hv[NMAX];
  __shared__ double pr[NMAX], pi[NMAX];  // the off-diagonal entries g of the Hermitian tridiagonal matrix, then the phases
  __shared__ double ur[NMAX], ui[NMAX], qr[NMAX], qi[NMAX];
  __shared__ double pt[4 * NMAX];        // the two halves' partial sums (re, im); (c_i, s_i) of a QL iteration
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

  // ---- 1. load both upper triangles, mirror A with conjugation, scan, scale ------------------------------------------------------
  double mxa = 0.0, mxb = 0.0, bad = 0.0;
  for (int j = hh; j < n; j += 2) {
    if (r <= j) {
      const size_t at = 2 * (r + (size_t)j * lda), bt = 2 * (r + (size_t)j * ldb);
      const double xr = ak[at], yr = bk[bt];
      const double xi = r < j ? ak[at + 1] : 0.0, yi = r < j ? bk[bt + 1] : 0.0;   // Im of the diagonals is not read
      if (!(fabs(xr) <= DBL_MAX) || !(fabs(xi) <= DBL_MAX) || !(fabs(yr) <= DBL_MAX) || !(fabs(yi) <= DBL_MAX)) bad = 1.0;
      else {
        mxa = fmax(mxa, fmax(fabs(xr), fabs(xi)));
        mxb = fmax(mxb, fmax(fabs(yr), fabs(yi)));
      }
      Sr[r + j * LD] = xr;
      Si[r + j * LD] = xi;
      Sr[j + r * LD] = xr;
      Si[j + r * LD] = -xi;
      Ur[r + j * LD] = yr;
      Ui[r + j * LD] = yi;
    }
  }
  bad = block_max<NT>(bad, red[0]);
  mxa = block_max<NT>(mxa, red[1]);
  mxb = block_max<NT>(mxb, red[2]);      // (the barriers also publish the loaded entries)
  if (bad != 0.0) return fail_block(k, EIGX_ERR_NONFINITE, row, r, wk, info, first);   // uniform; b is as it was passed
  // A by 2^-exa, B by 2^-exb with exb even: the factor of the caller's B is 2^(exb / 2) times the computed one
  const int exa = scale_exponent(mxa, false), exb = scale_exponent(mxb, true);
  if (exa != 0 && r < n) {
    const double sigma = ldexp(1.0, -exa);
    for (int j = hh; j < n; j += 2) { Sr[r + j * LD] *= sigma; Si[r + j * LD] *= sigma; }
  }
  if (exb != 0 && r < n) {
    const double sigma = ldexp(1.0, -exb);
    for (int j = hh; j < n; j += 2)
      if (r <= j) { Ur[r + j * LD] *= sigma; Ui[r + j * LD] *= sigma; }
  }
  if (row) perm[r] = r;
  __syncthreads();

  // ---- 2. B = U^H U, right-looking: two barriers per column ------------------------------------------------------------------
  bool spd = true;
  for (int c = 0; c < n; ++c) {
    const double p = Ur[c + c * LD];
    if (!(p > 0.0) || !(p <= DBL_MAX)) {   // the rule of eigx_zchol_dev (uniform)
      spd = false;
      break;
    }
    const double s = sqrt(p);
    if (row && r > c) {
      Ur[c + r * LD] = Ur[c + r * LD] / s;
      Ui[c + r * LD] = Ui[c + r * LD] / s;
    }
    __syncthreads();
    if (tid == 0) Ur[c + c * LD] = s;      // (every thread has read the pivot; nothing below reads the diagonal)
    if (r > c && r < n) {                  // the trailing block, lane = row: U(r, j) -= conj(U(c, r)) U(c, j), j >= r
      const double vr = Ur[c + r * LD], vi = Ui[c + r * LD];
      for (int j = c + 1 + hh; j < n; j += 2) {
        const double ujr = Ur[c + j * LD], uji = Ui[c + j * LD], xr = Ur[r + j * LD], xi = Ui[r + j * LD];
        if (r <= j) Ur[r + j * LD] = fma(-vi, uji, fma(-vr, ujr, xr));
        if (r < j) Ui[r + j * LD] = fma(vi, ujr, fma(-vr, uji, xi));   // (the diagonal stays real: its Im is left alone)
      }
    }
    __syncthreads();
  }
  if (!spd) return fail_block(k, EIGX_ERR_NOT_SPD, row, r, wk, info, first);

  // ---- 3. C = U^-H A U^-1: X = U^-H A down the columns (lane = column), C = X U^-1 along the rows (lane = row) ------------------
  if (row) zsolve_ut<LD, true>(n, Ur, Ui, Sr + r * LD, Si + r * LD, 1);
  __syncthreads();
  if (row) zsolve_ut<LD, false>(n, Ur, Ui, Sr + r, Si + r, LD);
  __syncthreads();
  // the upper triangle over the lower one with conjugation (the reduction wants C(r, c) and conj(C(c, r)) to be one number),
  // a real diagonal, scan, scale
  double mxc = 0.0;
  if (r < n) {
    for (int j = hh; j < n; j += 2) {
      if (r <= j) {
        const double xr = Sr[r + j * LD], xi = r < j ? Si[r + j * LD] : 0.0;
        if (!(fabs(xr) <= DBL_MAX) || !(fabs(xi) <= DBL_MAX)) bad = 1.0;
        else mxc = fmax(mxc, fmax(fabs(xr), fabs(xi)));
        Si[r + j * LD] = xi;
        Sr[j + r * LD] = xr;
        Si[j + r * LD] = -xi;
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
    for (int j = hh; j < n; j += 2) { Sr[r + j * LD] *= sigma; Si[r + j * LD] *= sigma; }
  }
  __syncthreads();

  // ---- 4. tridiagonalisation, phase chain, Q D in place, implicit QL (batch_common.h) ---------------------------------------
  if (herm_tridiag_ql<NMAX>(n, want_vec, Sr, Si, d, e, hv, pr, pi, ur, ui, qr, qi, pt, red, ctl, msk) == ST_FAIL)   // uniform
    return fail_block(k, EIGX_ERR_INTERNAL, row, r, wk, info, first);
  if (row) {
    const int rank = ascending_rank(n, d, r);
    perm[rank] = r;
    wk[rank] = ldexp(d[r], exa - exb + exc);   // C = 2^(exb - exa - exc) times the matrix that was solved
  }
  if (tid == 0 && info) info[k] = 0;

  // ---- 5. Z = U^-1 Y down the columns (lane = column), unscale, store -----------------------------------------------------------
  if (want_vec && row) zsolve_u<LD>(n, Ur, Ui, Sr + r * LD, Si + r * LD);
  __syncthreads();
  if (r < n) {
    if (want_vec) {
      double* zk = z + ds.off_z;
      for (int j = hh; j < n; j += 2) {
        const int c = perm[j];
        const size_t at = 2 * (r + (size_t)j * ldz);
        zk[at] = ldexp(Sr[r + c * LD], -(exb / 2));
        zk[at + 1] = ldexp(Si[r + c * LD], -(exb / 2));
      }
    }
    for (int j = hh; j < n; j += 2) {
      if (r <= j) {
        const size_t at = 2 * (r + (size_t)j * ldb);
        bk[at] = ldexp(Ur[r + j * LD], exb / 2);
        bk[at + 1] = r < j ? ldexp(Ui[r + j * LD], exb / 2) : 0.0;
      }
    }
  }
}

// the n-classes 32 and 64: the frame plans with top = 96 and a cutoff of at most 64, so the class of 96 stays empty
void hgvbatch_launch(int nclass, int count, const VbPencilDesc* desc, const VbArgs& g, hipStream_t st, unsigned long long* first) {
  const auto go = [&](auto nmax) {
    constexpr int NMAX = decltype(nmax)::value;
    hipLaunchKernelGGL(hgvbatch_kernel<NMAX>, dim3((unsigned)count), dim3(2 * NMAX), 0, st, desc, (const double*)g.a, g.b, g.w, g.z,
                       (int)(g.mode == 'A'), g.info, first);
  };
  if (nclass <= 32) go(std::integral_constant<int, 32>());
  else if (nclass <= EIGX_HGBATCH_NMAX) go(std::integral_constant<int, EIGX_HGBATCH_NMAX>());
}
// above the cutoff: block k as a uniform batch of one pencil through hgbatch_solve_one (hgbatch.hip)
int hgvbatch_solve_one(Context& ctx, const VbArgs& g, int k) {
  const int n = g.n[k];
  const bool want_vec = g.mode == 'A';
  const BatchArgs one{n, 1, g.block(g.a, g.off_a[k]), g.lda[k], 0, g.block(g.b, g.off_b[k]), g.ldb[k], 0, g.w + g.off_w[k], n,
                      want_vec ? g.block(g.z, g.off_z[k]) : nullptr, want_vec ? g.ldz[k] : n, 0, g.mode, nullptr, 16, true};
  return hgbatch_solve_one(ctx, one, 0);
}
// the largest n the kernels serve: key 24 (at most EIGX_HGBATCH_NMAX = 64)
int hgvbatch_cutoff() { return std::min(get_hgbatch_nmax(), EIGX_HGBATCH_NMAX); }

VbArgs hgvbatch_args(int batch, const int* n, double* a, const int64_t* off_a, const int* lda, double* b, const int64_t* off_b,
                     const int* ldb, double* w, const int64_t* off_w, double* z, const int64_t* off_z, const int* ldz, char mode,
                     int* info) {
  VbArgs g{batch, n, a, off_a, lda, w, off_w, z, off_z, ldz, mode, info, 16};
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

// EXTENSION: `batch` Hermitian-definite pencils of their own sizes (one GPU; a, b, z interleaved complex; offsets and leading
// dimensions in complex elements); see vbatch_frame_host / vbatch_frame_dev (batch_frame.hip)
int eigx_hgev_vbatch(int batch, const int* n, double* a, const int64_t* off_a, const int* lda, double* b, const int64_t* off_b,
                     const int* ldb, double* w, const int64_t* off_w, double* z, const int64_t* off_z, const int* ldz, char mode,
                     int* info) {
  const VbArgs g = hgvbatch_args(batch, n, a, off_a, lda, b, off_b, ldb, w, off_w, z, off_z, ldz, mode, info);
  return eigx_guard(g_ctx, [&] {
    return vbatch_frame_host(g_ctx, g, hgvbatch_cutoff(), 96, (VbPencilLaunch)hgvbatch_launch, hgvbatch_solve_one);
  });
}
int eigx_hgev_vbatch_dev(int batch, const int* n, double* a_dev, const int64_t* off_a, const int* lda, double* b_dev,
                         const int64_t* off_b, const int* ldb, double* w_dev, const int64_t* off_w, double* z_dev,
                         const int64_t* off_z, const int* ldz, char mode, int* info_dev) {
  const VbArgs g = hgvbatch_args(batch, n, a_dev, off_a, lda, b_dev, off_b, ldb, w_dev, off_w, z_dev, off_z, ldz, mode, info_dev);
  return eigx_guard(g_ctx, [&] {
    return vbatch_frame_dev(g_ctx, g, hgvbatch_cutoff(), 96, (VbPencilLaunch)hgvbatch_launch, hgvbatch_solve_one);
  });
}

}  // extern "C"
