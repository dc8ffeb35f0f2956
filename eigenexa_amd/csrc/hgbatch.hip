// hgbatch.hip -- eigx_hgev_batch and eigx_hgev_vbatch (EXTENSIONS, not in the reference): many small Hermitian-definite pencils
// A x = lambda B x (n <= EIGX_HGBATCH_NMAX) in one call, one workgroup per pencil, both matrices resident in LDS from load to
// store.  Uniform: one size, block k a stride on from block k - 1, one launch.  Ragged (section 8m): every
// block with its own order n[k], leading dimensions and offsets (in complex elements) into one interleaved buffer each for a, b
// and z and one real buffer for w, one launch per non-empty n-class (32, 64).  Both run the one kernel below, which differs
// between them in where a workgroup finds its block (UniformPencils, RaggedPencils) and in nothing else, so a block's w, z
// and U are bit for bit the same from either entry.  The Cholesky route of gbatch.hip over complex numbers, on the split
// planes and the reduction of hbatch.hip:
//   load the upper triangles of A (mirrored with conjugation) and B (interleaved complex; of the diagonals the real parts
//   only), scan both for NaN / Inf, scale each by a power of two (B by an even one)
//   -> B = U^H U, upper and right-looking, one column per step; the diagonal of U is real
//   -> C = U^-H A U^-1: a forward substitution down every column, then the same along every row; mirrored, scanned, scaled
//   -> Hermitian tridiagonalisation, phase chain, Q D in place, implicit QL on the real (d, e): herm_tridiag_ql of
//      batch_common.h, the code eigx_h_batch runs
//   -> sort ascending, Z = U^-1 Y by a backward substitution down every column, unscale, store w, z and U (into b).
// No workgroup talks to another: no grid-wide barrier, no spin-wait, no atomics on the data.  Every sum is taken in an order
// that depends on n alone, so a pencil's result does not depend on its position in the batch or on the batch size.
// Pencils larger than the cutoff (eigx_tune key 24) go through hgev_range_dev (hgev.hip) one by one.
// Here: the kernel, the cutoff and what the frames of the batch families ask for (batch_frame.hip: checks, launch and failure
// word, the loop above the cutoff, the schedule of a ragged batch, host staging of a, b, z, w): the launches and the full-size
// solves of one pencil.
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

// (the substitutions zsolve_ut and zsolve_u: batch_solve.h)

// Where the pencil of a workgroup lies: the one thing in which the two entries differ.  The kernel takes one of these by value
// and reads where.block(blockIdx.x), the descriptor of the ragged frame (eigx_context.h: caller index k, n, leading dimensions,
// offsets in doubles from the entry's a, b, w, z).  Uniform: pencil k lies k strides on (strides in complex elements: the factor
// 2); ragged: the frame's descriptors of one n-class in device memory, one per workgroup.
struct UniformPencils {
  int n, lda, ldb, ldw, ldz;
  int64_t stride_a, stride_b, stride_z;
  __device__ VbPencilDesc block(int k) const {
    const int64_t k2 = 2 * (int64_t)k;
    return {k, n, lda, ldb, ldz, k2 * stride_a, k2 * stride_b, (int64_t)k * ldw, k2 * stride_z};
  }
};
struct RaggedPencils {
  const VbPencilDesc* desc;
  __device__ VbPencilDesc block(int i) const { return desc[i]; }
};

// One workgroup of 2 NMAX threads per pencil (NMAX = 32, 64: the n-classes), which ends with it: thread (r, hh) = (row, half) as
// in every batch kernel.  Where = UniformPencils or RaggedPencils; the descriptor's offsets of a, b and z count
// doubles.  The split planes Sr, Si(LD, NMAX) hold A, then C, then Q, then Z; Ur, Ui(LD, NMAX) hold B, then its factor (upper
// triangle; the strict lower triangle is never read, the imaginary part of the diagonal never computed); column-major with
// LD = NMAX + 1, the access patterns of hbatch_kernel: lane = row at a fixed column is stride 1, lane = column is a stride of LD
// doubles, an entry of U that all lanes read is a broadcast.
template <int NMAX, class Where>
__global__ __launch_bounds__(2 * NMAX) void hgbatch_kernel(Where where, const double* __restrict__ a, double* __restrict__ b,
                                                           double* __restrict__ w, double* __restrict__ z, int want_vec,
                                                           int* __restrict__ info, unsigned long long* __restrict__ first) {
  const VbPencilDesc ds = where.block(blockIdx.x);   // the same for every thread of the workgroup
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
  if (bad != 0.0) return fail_block(k, EIGX_ERR_NONFINITE, row, r, wk, info, first);   // (every thread agrees); b is as it was passed
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
    if (!(p > 0.0) || !(p <= DBL_MAX)) {   // the rule of eigx_zchol_dev (every thread agrees)
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
  // (every thread agrees: B was too close to singular for C to be formed)
  if (bad != 0.0) return fail_block(k, EIGX_ERR_NOT_SPD, row, r, wk, info, first);
  const int exc = scale_exponent(mxc, false);
  if (exc != 0 && r < n) {
    const double sigma = ldexp(1.0, -exc);
    for (int j = hh; j < n; j += 2) { Sr[r + j * LD] *= sigma; Si[r + j * LD] *= sigma; }
  }
  __syncthreads();

  // ---- 4. tridiagonalisation, phase chain, Q D in place, implicit QL (batch_common.h) ---------------------------------------
  if (herm_tridiag_ql<NMAX>(n, want_vec, Sr, Si, d, e, hv, pr, pi, ur, ui, qr, qi, pt, red, ctl, msk) == ST_FAIL)
    return fail_block(k, EIGX_ERR_INTERNAL, row, r, wk, info, first);   // (every thread agrees)
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

int g_hgbatch_nmax = EIGX_HGBATCH_NMAX;   // key 24: largest n served by the batch kernel

// One workgroup per pencil of the uniform batch / per descriptor of the ragged batch's class.  The n-classes are 32 and 64
// (with_n_class serves the families whose largest class is 96 or 128); the ragged frame plans with top = 96 and a cutoff of at
// most 64, so its class of 96 stays empty.
void hgbatch_launch(const BatchArgs& g, hipStream_t st, unsigned long long* first) {
  const UniformPencils where{g.n, g.lda, g.ldb, g.ldw, g.ldz, g.stride_a, g.stride_b, g.stride_z};
  const auto go = [&](auto nmax) {
    constexpr int NMAX = decltype(nmax)::value;
    hipLaunchKernelGGL((hgbatch_kernel<NMAX, UniformPencils>), dim3((unsigned)g.batch), dim3(2 * NMAX), 0, st, where,
                       (const double*)g.a, g.b, g.w, g.z, (int)(g.mode == 'A'), g.info, first);
  };
  if (g.n <= 32) go(std::integral_constant<int, 32>());
  else go(std::integral_constant<int, EIGX_HGBATCH_NMAX>());
}
void hgvbatch_launch(int nclass, int count, const VbPencilDesc* desc, const VbArgs& g, hipStream_t st, unsigned long long* first) {
  const auto go = [&](auto nmax) {
    constexpr int NMAX = decltype(nmax)::value;
    hipLaunchKernelGGL((hgbatch_kernel<NMAX, RaggedPencils>), dim3((unsigned)count), dim3(2 * NMAX), 0, st,
                       RaggedPencils{desc}, (const double*)g.a, g.b, g.w, g.z, (int)(g.mode == 'A'), g.info, first);
  };
  if (nclass <= 32) go(std::integral_constant<int, 32>());
  else if (nclass <= EIGX_HGBATCH_NMAX) go(std::integral_constant<int, EIGX_HGBATCH_NMAX>());
}

// above the cutoff: hgev_range_dev with il = 1, iu = n; it takes every leading dimension >= n, so nothing is staged
int hgbatch_solve_one(Context& ctx, const BatchArgs& g, int k) {
  return hgev_range_dev(ctx, g.n, RangeWindow::index(1, g.n), g.block(g.a, g.stride_a, k), g.lda, g.block(g.b, g.stride_b, k), g.ldb,
                        g.w + (size_t)k * g.ldw, g.mode == 'A' ? g.block(g.z, g.stride_z, k) : nullptr, g.ldz, g.mode);
}
// block k of a ragged batch as a uniform batch of one pencil
int hgvbatch_solve_one(Context& ctx, const VbArgs& g, int k) {
  const int n = g.n[k];
  const bool want_vec = g.mode == 'A';
  const BatchArgs one{n, 1, g.block(g.a, g.off_a[k]), g.lda[k], 0, g.block(g.b, g.off_b[k]), g.ldb[k], 0, g.w + g.off_w[k], n,
                      want_vec ? g.block(g.z, g.off_z[k]) : nullptr, want_vec ? g.ldz[k] : n, 0, g.mode, nullptr, 16, true};
  return hgbatch_solve_one(ctx, one, 0);
}
// the largest n the kernels serve in a ragged batch: key 24 (at most EIGX_HGBATCH_NMAX = 64)
int hgvbatch_cutoff() { return std::min(g_hgbatch_nmax, EIGX_HGBATCH_NMAX); }

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

int set_hgbatch_nmax(int v) {
  if (v < 0 || v > EIGX_HGBATCH_NMAX) return -1;
  const int old = g_hgbatch_nmax;
  g_hgbatch_nmax = v;
  return old;
}
int get_hgbatch_nmax() { return g_hgbatch_nmax; }

}  // namespace eigx

using namespace eigx;

extern "C" {

// EXTENSION: `batch` Hermitian-definite pencils of one size (one GPU; a, b, z interleaved complex; lda, ldb, ldz and the strides
// in complex elements); see batch_frame_host / batch_frame_dev (batch_frame.hip)
int eigx_hgev_batch(int n, int batch, double* a, int lda, int64_t stride_a, double* b, int ldb, int64_t stride_b, double* w, int ldw,
                    double* z, int ldz, int64_t stride_z, char mode, int* info) {
  const BatchArgs g{n, batch, a, lda, stride_a, b, ldb, stride_b, w, ldw, z, ldz, stride_z, mode, info, 16, true};
  return eigx_guard(g_ctx, [&] { return batch_frame_host(g_ctx, g, g_hgbatch_nmax, hgbatch_launch, hgbatch_solve_one); });
}
int eigx_hgev_batch_dev(int n, int batch, double* a_dev, int lda, int64_t stride_a, double* b_dev, int ldb, int64_t stride_b,
                        double* w_dev, int ldw, double* z_dev, int ldz, int64_t stride_z, char mode, int* info_dev) {
  const BatchArgs g{n, batch, a_dev, lda, stride_a, b_dev, ldb, stride_b, w_dev, ldw, z_dev, ldz, stride_z, mode, info_dev, 16, true};
  return eigx_guard(g_ctx, [&] { return batch_frame_dev(g_ctx, g, g_hgbatch_nmax, hgbatch_launch, hgbatch_solve_one); });
}

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
