// ztri.hip -- complex triangular stages of the Cholesky-route Hermitian generalised solver (EXTENSION, one GPU; LAPACK
// uplo = 'U').  The complex siblings of tri.hip, on split planes (Re and Im of a matrix as two real column-major arrays
// of one leading dimension, ZPlanes), as hgev.hip and herm.hip work:
//   zchol_upper_dev    : B = U^H U, U in place in the upper triangle, real positive diagonal (role of zpotrf)
//   ztri_inverses_dev  : the inverses of the NB-wide diagonal blocks of U (pool buffer hgevr.inv)
//   ztrsm_upper_dev    : X <- op(U)^-1 X by block inversion, op = none ('N') or conjugate transpose ('C') (role of ztrsm)
//   hgev_reduce_dev    : upper(C) = U^-H A U^-1 (role of zhegst, itype 1) by two solves with U^H and a conjugate transpose
// NB is the outer block width, eigx_tune key 20, shared with tri.hip.  The structure is that of tri.hip step for step;
// everything of O(n^3) is a complex product on the planes, which zgemm_planes (zplanes.hip) runs as FOUR real fp64 MFMA
// GEMMs with beta accumulation (Cr = Ar Br - Ai Bi, Ci = Ar Bi + Ai Br; a conjugate-transposed left operand flips the sign
// of Ai).  The planes, their conversions and the conjugate transpose come from zplanes.hip as well.  Stacking K to
// [Ur; Ui] instead would need the row panel of every step packed twice (rows are the K index of a transposed operand, so
// the two planes of a panel are not contiguous in K) to save two of the four passes over C; with K = NB = 256 a pass over
// C is 16 bytes per 512 flops of a product, far below what the GEMM is bound by.
// Nothing below the diagonal of B / U is read; what the kernels write there is unspecified.  Im of B's diagonal is not
// read; Im of U's diagonal is written as 0.
#include "eigx_context.h"
#include "../../include/eigenexa_amd.h"
#include <algorithm>
#include <cfloat>

namespace eigx {

namespace {

constexpr int TB = 64;             // inner block = one column per lane of a wave
constexpr int SP = TB * (TB + 1);  // doubles of one LDS plane, rows padded by one (conflict-free in both directions)
// dynamic LDS of the diagonal-block kernels: two padded planes + the double-buffered pivot row (re | im): 68 608 bytes,
// more than the 64 KiB a kernel gets without asking
constexpr size_t ZDIAG_SHM = (size_t)(2 * SP + 4 * TB) * sizeof(double);
// ... and of the row-panel kernel: the inverse and one tile, two planes each
constexpr size_t ZROW_SHM = (size_t)4 * TB * TB * sizeof(double);

// S(i, c) = block(i, c) for i <= c < nb, the identity beyond nb, zero below the diagonal; Im of the diagonal := 0.  One
// wave; a column per step, lanes along the rows (coalesced).
__device__ inline void zload_upper64(double* Sr, double* Si, const double* __restrict__ srcr, const double* __restrict__ srci,
                                     int ld, int nb, int lane) {
  for (int c = 0; c < TB; ++c) {
    const bool in = lane <= c && c < nb;
    Sr[lane * (TB + 1) + c] = in ? srcr[(size_t)c * ld + lane] : (lane == c ? 1.0 : 0.0);
    Si[lane * (TB + 1) + c] = (in && lane != c) ? srci[(size_t)c * ld + lane] : 0.0;
  }
}

// Both planes of a lane's column in registers are 256 registers before any temporary: the compiler then spills (the
// factorisation) or leaves the arrays in scratch memory (the inversion).  So the factorisation runs on TWO waves, wave p
// holding plane p of the columns (64 doubles per lane, as the real kernel), and the inversion keeps Im in LDS.
// The steps of both are compile-time recursions, not loops: twice the body of the real kernel puts the unrolled outer
// loop past the compiler's size limit for a pragma, and a loop left rolled indexes the register array at run time,
// which sends it to scratch memory as well.

// Right-looking U^H U factorisation of a 64 x 64 block: c[i] = plane p of element (i, lane).  An update
// A(i, j) -= conj(U(k, i)) U(k, j) changes Re from Re alone and Im from Im alone once row k is known to everybody, and
// row k goes through LDS (rr = Re from wave 0, ri = Im from wave 1; double-buffered: one barrier per step).  Entries
// below the diagonal take part as dead weight and are never read as part of U.  The pivot is the REAL part of the
// diagonal entry alone (rounding may leave a residue in its imaginary part; U's diagonal is written as (s, 0)).
// bad: a pivot that is not > 0 or not finite (replaced by 1); both waves see the same.
template <int K>
__device__ __forceinline__ void zchol64_step(double (&c)[TB], double* row, int lane, int p, bool& bad) {
  double* rr = row + (K & 1) * 2 * TB;
  double* ri = rr + TB;
  (p ? ri : rr)[lane] = c[K];
  __syncthreads();
  const double d = rr[K];
  double s = 1.0;
  if (!(d > 0.0) || !(d <= DBL_MAX)) bad = true;
  else s = sqrt(d);
  const double rinv = 1.0 / s;
  // (loaded before the selects: a load inside an arm of ?: becomes a branch, and with 64 steps of basic blocks the
  // compiler sinks the updates of c[i] down to their first use and keeps every row alive until then)
  const double okr = rr[lane] * rinv, oki = ri[lane] * rinv;
  const double bkr = (lane == K) ? s : okr;
  const double bki = (lane == K) ? 0.0 : oki;
  c[K] = p ? bki : bkr;
  // Re: c -= ar bkr + ai bki;  Im: c -= ar bki - ai bkr   with (ar, ai) = U(k, i)
  const double x = p ? bki : bkr, y = p ? -bkr : bki;
#pragma unroll
  for (int i = K + 1; i < TB; ++i) c[i] -= (rr[i] * rinv) * x + (ri[i] * rinv) * y;
  if constexpr (K + 1 < TB) zchol64_step<K + 1>(c, row, lane, p, bad);
}

// Column `lane` of the inverse of the upper triangular S (real diagonal; nothing below the diagonal is read) by back
// substitution, rows from the last to the first; the row of S is a broadcast read.  Re of the column in vr (registers), Im
// in LDS and IN PLACE (two 64-double arrays here stay in scratch memory): once every lane has read row I of S, Si(I, lane)
// takes Im of V(I, lane); the rows still to come read S only above row I.  One wave runs in step, and the barriers keep
// the compiler from moving the store above the reads.
template <int I>
__device__ __forceinline__ void zinv64_row(const double* Sr, double* Si, double (&vr)[TB], int lane) {
  double sr = (I == lane) ? 1.0 : 0.0, si = 0.0;
#pragma unroll
  for (int k = I + 1; k < TB; ++k) {
    const double ur = Sr[I * (TB + 1) + k], ui = Si[I * (TB + 1) + k];
    const double vi = Si[k * (TB + 1) + lane];
    sr -= ur * vr[k] - ui * vi;
    si -= ur * vi + ui * vr[k];
  }
  const double d = Sr[I * (TB + 1) + I];
  vr[I] = sr / d;
  __syncthreads();
  Si[I * (TB + 1) + lane] = si / d;
  __syncthreads();
  if constexpr (I > 0) zinv64_row<I - 1>(Sr, Si, vr, lane);
}

// Diagonal block [k0, k0 + nb) of the Cholesky factorisation: U_kk in place.  stat[0] = 1 on a breakdown.  Two waves:
// wave p loads, factors and stores plane p.  The inverse of the block is a launch of its own (zchol_inv_block_kernel).
__global__ __launch_bounds__(2 * TB) void zchol_diag_upper_kernel(double* __restrict__ Br, double* __restrict__ Bi, int ldb, int k0,
                                                                  int nb, int* __restrict__ stat) {
  extern __shared__ double zlds[];
  const int lane = threadIdx.x & (TB - 1), p = threadIdx.x >> 6;
  double* S = zlds + p * SP;
  double* row = zlds + 2 * SP;
  double* blk = (p ? Bi : Br) + (size_t)k0 * ldb + k0;
  // S(i, c) = block(i, c) for i <= c < nb, the identity beyond nb, zero below the diagonal; Im of the diagonal := 0
  for (int c = 0; c < TB; ++c) {
    const bool in = lane <= c && c < nb && !(p && lane == c);
    S[lane * (TB + 1) + c] = in ? blk[(size_t)c * ldb + lane] : ((!p && lane == c) ? 1.0 : 0.0);
  }
  __syncthreads();
  bool bad = false;
  double c[TB];
#pragma unroll
  for (int i = 0; i < TB; ++i) c[i] = S[i * (TB + 1) + lane];
  zchol64_step<0>(c, row, lane, p, bad);
  __syncthreads();
#pragma unroll
  for (int i = 0; i < TB; ++i) S[i * (TB + 1) + lane] = c[i];
  __syncthreads();
  for (int q = 0; q < nb; ++q)
    if (lane <= q) blk[(size_t)q * ldb + lane] = S[lane * (TB + 1) + q];
  if (bad && threadIdx.x == 0) stat[0] = 1;
}

// Vt = the inverse of the factored diagonal block [k0, k0 + nb), ROW-major 64 x 64 planes (Vt[p * 4096 + k * 64 + i] =
// plane p of inv(U_kk)(k, i)), as zchol_row_panel_kernel reads it.
__global__ __launch_bounds__(TB) void zchol_inv_block_kernel(const double* __restrict__ Br, const double* __restrict__ Bi, int ldb,
                                                             int k0, int nb, double* __restrict__ Vt) {
  extern __shared__ double zlds[];
  double* Sr = zlds;
  double* Si = zlds + SP;
  const int lane = threadIdx.x;
  zload_upper64(Sr, Si, Br + (size_t)k0 * ldb + k0, Bi + (size_t)k0 * ldb + k0, ldb, nb, lane);
  __syncthreads();
  double vr[TB];
  zinv64_row<TB - 1>(Sr, Si, vr, lane);
#pragma unroll
  for (int i = 0; i < TB; ++i) {
    Vt[i * TB + lane] = vr[i];
    Vt[TB * TB + i * TB + lane] = Si[i * (TB + 1) + lane];
  }
}

// Row panel of one 64-wide step: B(k0 : k0 + nb, c0 + 64 t : ...) <- inv(U_kk)^H B(...), one 64 x 64 tile per workgroup.
// out(i, c) = sum_k conj(V(k, i)) T(k, c): thread = row i, a wave = 16 columns; V(k, .) is read along the lanes, T(k, c)
// is a broadcast.
__global__ __launch_bounds__(256) void zchol_row_panel_kernel(double* __restrict__ Br, double* __restrict__ Bi, int ldb, int k0,
                                                              int nb, int c0, int ncols, const double* __restrict__ Vt) {
  extern __shared__ double zlds[];
  double* Vsr = zlds;                 // Vs[k * 64 + i] = V(k, i)
  double* Vsi = zlds + TB * TB;
  double* Tsr = zlds + 2 * TB * TB;   // Ts[c * 64 + k] = B(k0 + k, c0 + cb + c)
  double* Tsi = zlds + 3 * TB * TB;
  const int tid = threadIdx.x;
  const int cb = blockIdx.x * TB;
  for (int q = tid; q < TB * TB; q += 256) {
    const int k = q & (TB - 1), c = q >> 6;
    Vsr[q] = Vt[q];
    Vsi[q] = Vt[TB * TB + q];
    const bool in = k < nb && cb + c < ncols;
    const size_t o = (size_t)(c0 + cb + c) * ldb + k0 + k;
    Tsr[q] = in ? Br[o] : 0.0;
    Tsi[q] = in ? Bi[o] : 0.0;
  }
  __syncthreads();
  const int i = tid & (TB - 1), cw = (tid >> 6) * 16;
  double accr[16], acci[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) accr[t] = acci[t] = 0.0;
  for (int k = 0; k < TB; ++k) {
    const double vr = Vsr[k * TB + i], vi = Vsi[k * TB + i];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const double tr = Tsr[(cw + t) * TB + k], ti = Tsi[(cw + t) * TB + k];
      accr[t] += vr * tr + vi * ti;
      acci[t] += vr * ti - vi * tr;
    }
  }
  if (i < nb) {
#pragma unroll
    for (int t = 0; t < 16; ++t)
      if (cb + cw + t < ncols) {
        const size_t o = (size_t)(c0 + cb + cw + t) * ldb + k0 + i;
        Br[o] = accr[t];
        Bi[o] = acci[t];
      }
  }
}

// Inverses of all 64-wide diagonal blocks of U in one launch (block q of the grid: rows / columns [64 q, 64 q + 64)),
// written to their place inside the NB x NB inverse of outer block 64 q / NB (column-major, leading dimension NB), the
// imaginary plane `vplane` doubles behind the real one.
__global__ __launch_bounds__(TB) void ztri_inv_diag_kernel(const double* __restrict__ Ur, const double* __restrict__ Ui, int ldu,
                                                           int n, int NB, double* __restrict__ Vinv, size_t vplane) {
  extern __shared__ double zlds[];
  double* Sr = zlds;
  double* Si = zlds + SP;
  const int lane = threadIdx.x;
  const int k0 = blockIdx.x * TB, nb = (n - k0 < TB) ? n - k0 : TB;
  zload_upper64(Sr, Si, Ur + (size_t)k0 * ldu + k0, Ui + (size_t)k0 * ldu + k0, ldu, nb, lane);
  __syncthreads();
  double vr[TB];
  zinv64_row<TB - 1>(Sr, Si, vr, lane);
#pragma unroll
  for (int i = 0; i < TB; ++i) Sr[i * (TB + 1) + lane] = vr[i];
  __syncthreads();
  const int K = k0 / NB, off = k0 - K * NB;
  double* dst = Vinv + (size_t)K * NB * NB + (size_t)off * NB + off;
  for (int q = 0; q < nb; ++q)
    if (lane < nb) {
      dst[(size_t)q * NB + lane] = Sr[lane * (TB + 1) + q];
      dst[vplane + (size_t)q * NB + lane] = Si[lane * (TB + 1) + q];
    }
}

// the four kernels with dynamic LDS above 64 KiB ask for it once
void zlds_attributes() {
  static bool done = false;
  if (done) return;
  EIGX_HIP_CHECK(hipFuncSetAttribute((const void*)zchol_diag_upper_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ZDIAG_SHM));
  EIGX_HIP_CHECK(hipFuncSetAttribute((const void*)zchol_inv_block_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ZDIAG_SHM));
  EIGX_HIP_CHECK(hipFuncSetAttribute((const void*)ztri_inv_diag_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ZDIAG_SHM));
  EIGX_HIP_CHECK(hipFuncSetAttribute((const void*)zchol_row_panel_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ZROW_SHM));
  done = true;
}

}  // namespace

int zchol_upper_dev(Context& ctx, int n, const ZPlanes& B, int ldb) {
  hipStream_t st = ctx.stream;
  const int NB = get_tri_nb();
  zlds_attributes();
  int* stat = ctx.pool.get_t<int>("hgevr.stat", 4);
  double* Vt = ctx.pool.get_t<double>("hgevr.v64", (size_t)2 * TB * TB);
  EIGX_HIP_CHECK(hipMemsetAsync(stat, 0, 4 * sizeof(int), st));
  for (int p0 = 0; p0 < n; p0 += NB) {
    const int p1 = std::min(p0 + NB, n);
    for (int j0 = p0; j0 < p1; j0 += TB) {
      const int nb = std::min(TB, n - j0), j1 = j0 + nb;
      hipLaunchKernelGGL(zchol_diag_upper_kernel, dim3(1), dim3(2 * TB), ZDIAG_SHM, st, B.r, B.i, ldb, j0, nb, stat);
      if (j1 >= n) break;
      hipLaunchKernelGGL(zchol_inv_block_kernel, dim3(1), dim3(TB), ZDIAG_SHM, st, (const double*)B.r, (const double*)B.i, ldb, j0, nb, Vt);
      hipLaunchKernelGGL(zchol_row_panel_kernel, dim3(ceil_div(n - j1, TB)), dim3(256), ZROW_SHM, st, B.r, B.i, ldb, j0, nb, j1,
                         n - j1, (const double*)Vt);
      // the panel's remaining rows, all columns to the right: B(j1:p1, j1:n) -= U(j0:j1, j1:p1)^H U(j0:j1, j1:n)
      const ZPlanes U12 = B.at((size_t)j1 * ldb + j0);
      if (j1 < p1) zgemm_planes(st, 'C', p1 - j1, n - j1, nb, -1.0, U12, ldb, U12, ldb, 1.0, B.at((size_t)j1 * ldb + j1), ldb);
    }
    if (p1 < n) {
      // trailing update of the outer panel, tiles of the upper triangle only: B22 -= U12^H U12
      const ZPlanes U12 = B.at((size_t)p1 * ldb + p0);
      zgemm_planes(st, 'C', n - p1, n - p1, p1 - p0, -1.0, U12, ldb, U12, ldb, 1.0, B.at((size_t)p1 * ldb + p1), ldb, 1);
    }
  }
  int bad = 0;
  EIGX_HIP_CHECK(hipMemcpyAsync(&bad, stat, sizeof(int), hipMemcpyDeviceToHost, st));
  EIGX_HIP_CHECK(hipStreamSynchronize(st));
  return bad ? EIGX_ERR_NOT_SPD : EIGX_OK;
}

ZTriInv ztri_inverses_dev(Context& ctx, int n, const ZPlanes& U, int ldu) {
  hipStream_t st = ctx.stream;
  const int NB = get_tri_nb();
  zlds_attributes();
  const int nblk = ceil_div(n, NB), nfull = n / NB, Wl = n - nfull * NB;
  const size_t vp = (size_t)nblk * NB * NB;
  ZTriInv V;
  V.nb = NB;
  V.v.r = ctx.pool.get_t<double>("hgevr.inv", 2 * vp);
  V.v.i = V.v.r + vp;
  // U12 V22 of one level: at most n / (2 w) blocks of w x w, w < NB; two planes
  const size_t tp = (size_t)n * NB + (size_t)NB * NB;
  ZPlanes T;
  T.r = ctx.pool.get_t<double>("hgevr.invt", 2 * tp);
  T.i = T.r + tp;
  EIGX_HIP_CHECK(hipMemsetAsync(V.v.r, 0, 2 * vp * sizeof(double), st));
  hipLaunchKernelGGL(ztri_inv_diag_kernel, dim3(ceil_div(n, TB)), dim3(TB), ZDIAG_SHM, st, (const double*)U.r, (const double*)U.i,
                     ldu, n, NB, V.v.r, vp);
  // `batch` pairs (left block of width w at local offset o + 2 w q, right block of width wr behind it) in each of `batch2`
  // outer blocks from K0 on: V12 = -V11 (U12 V22)
  auto pairs = [&](int K0, int o, int w, int wr, int batch, int batch2) {
    if (batch <= 0 || batch2 <= 0 || wr <= 0) return;
    const size_t r0 = (size_t)K0 * NB + o;
    const size_t oU12 = r0 + (r0 + w) * ldu;
    const size_t ob = (size_t)K0 * NB * NB;
    const size_t oV11 = ob + o + (size_t)o * NB, oV22 = ob + (o + w) + (size_t)(o + w) * NB, oV12 = ob + o + (size_t)(o + w) * NB;
    const long sU = 2L * w * (ldu + 1), sV = 2L * w * (NB + 1), sT = (long)w * w;
    const long sU2 = (long)NB * (ldu + 1), sV2 = (long)NB * NB, sT2 = sT * batch;
    zgemm_planes(st, 'N', w, wr, wr, 1.0, U.at(oU12), ldu, V.v.at(oV22), NB, 0.0, T, w, 0,
                 ZBatch{batch, sU, sV, sT, batch2, sU2, sV2, sT2});
    zgemm_planes(st, 'N', w, wr, w, -1.0, V.v.at(oV11), NB, T, w, 0.0, V.v.at(oV12), NB, 0,
                 ZBatch{batch, sV, sT, sV, batch2, sV2, sT2, sV2});
  };
  for (int w = TB; w < NB; w *= 2) {
    const int npf = NB / (2 * w), rem = NB - npf * 2 * w;       // the full outer blocks
    pairs(0, 0, w, w, npf, nfull);
    if (rem > w) pairs(0, npf * 2 * w, w, rem - w, 1, nfull);
    const int npl = Wl / (2 * w), reml = Wl - npl * 2 * w;      // the last, narrower one
    pairs(nfull, 0, w, w, npl, 1);
    if (reml > w) pairs(nfull, npl * 2 * w, w, reml - w, 1, 1);
  }
  return V;
}

void ztrsm_upper_dev(Context& ctx, char trans, int n, int nrhs, const ZPlanes& U, int ldu, const ZPlanes& X, int ldx,
                     const ZTriInv& V, bool upper_only) {
  if (nrhs <= 0) return;
  if (trans != 'C' || nrhs != n) upper_only = false;
  hipStream_t st = ctx.stream;
  const int NB = V.nb, nblk = ceil_div(n, NB);
  ZPlanes t;
  t.r = ctx.pool.get_t<double>("hgevr.xk", (size_t)2 * NB * nrhs);
  t.i = t.r + (size_t)NB * nrhs;
  for (int q = 0; q < nblk; ++q) {
    const int K = (trans == 'C') ? q : nblk - 1 - q;           // U^H is lower triangular: forwards; U: backwards
    const int k0 = K * NB, w = std::min(NB, n - k0), k1 = k0 + w;
    // upper_only (trans 'C', X square): block row K of the result is wanted from column k0 on, and the rows below it want
    // still fewer columns, so the columns before k0 drop out of this and every later step (2/3 of the flops remain)
    const int c0 = upper_only ? k0 : 0, nc = nrhs - c0;
    const ZPlanes Xc = X.at((size_t)c0 * ldx);
    zgemm_planes(st, trans, w, nc, w, 1.0, V.v.at((size_t)K * NB * NB), NB, Xc.at(k0), ldx, 0.0, t, NB);
    EIGX_HIP_CHECK(hipMemcpy2DAsync(Xc.r + k0, (size_t)ldx * 8, t.r, (size_t)NB * 8, (size_t)w * 8, (size_t)nc,
                                    hipMemcpyDeviceToDevice, st));
    EIGX_HIP_CHECK(hipMemcpy2DAsync(Xc.i + k0, (size_t)ldx * 8, t.i, (size_t)NB * 8, (size_t)w * 8, (size_t)nc,
                                    hipMemcpyDeviceToDevice, st));
    if (trans == 'C') zgemm_planes(st, 'C', n - k1, nc, w, -1.0, U.at((size_t)k1 * ldu + k0), ldu, t, NB, 1.0, Xc.at(k1), ldx);
    else zgemm_planes(st, 'N', k0, nc, w, -1.0, U.at((size_t)k0 * ldu), ldu, t, NB, 1.0, Xc, ldx);
  }
}

// upper(C) = U^-H A U^-1 (below the diagonal C is unspecified); the planes of A hold the full Hermitian matrix and are
// overwritten.  4 x 5/3 n^3 real flops: A <- U^-H A, C = A^H, C <- U^-H C on the block columns that reach the upper triangle.
void hgev_reduce_dev(Context& ctx, int n, const ZPlanes& A, int lda, const ZPlanes& U, int ldu, const ZTriInv& V, const ZPlanes& C,
                     int ldc) {
  ztrsm_upper_dev(ctx, 'C', n, n, U, ldu, A, lda, V);
  zconj_transpose(ctx.stream, n, A, lda, C, ldc);
  ztrsm_upper_dev(ctx, 'C', n, n, U, ldu, C, ldc, V, true);   // eigen_h reads the upper triangle only
}

}  // namespace eigx

using namespace eigx;

extern "C" {

int eigx_zchol_dev(int n, double* b_dev, int ldb) {
  if (!g_ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  if (n <= 0 || !b_dev || ldb < n) return EIGX_ERR_BAD_ARG;
  if (g_ctx.grid.nranks != 1) return EIGX_ERR_INTERNAL;
  return eigx_guard(g_ctx, [&] {
    EIGX_HIP_CHECK(hipSetDevice(g_ctx.device));
    EIGX_HIP_CHECK(hipStreamSynchronize(nullptr));
    hipStream_t st = g_ctx.stream;
    const int ld = pad_ld(n);
    const ZPlanes U = zplanes(g_ctx, "hgevr.u", ld, n);
    zsplit(st, b_dev, ldb, n, n, true, U, ld);
    const int rc = zchol_upper_dev(g_ctx, n, U, ld);
    zjoin(st, U, ld, n, n, true, b_dev, ldb);
    EIGX_HIP_CHECK(hipStreamSynchronize(st));
    return rc;
  });
}

int eigx_ztrsm_upper_dev(char trans, int n, int nrhs, const double* u_dev, int ldu, double* x_dev, int ldx) {
  if (!g_ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  trans = upper_case(trans);
  if (n <= 0 || nrhs < 0 || !u_dev || !x_dev || ldu < n || ldx < n || (trans != 'N' && trans != 'C')) return EIGX_ERR_BAD_ARG;
  if (g_ctx.grid.nranks != 1) return EIGX_ERR_INTERNAL;
  return eigx_guard(g_ctx, [&] {
    EIGX_HIP_CHECK(hipSetDevice(g_ctx.device));
    EIGX_HIP_CHECK(hipStreamSynchronize(nullptr));
    if (nrhs == 0) return EIGX_OK;
    hipStream_t st = g_ctx.stream;
    const int ld = pad_ld(n);
    const ZPlanes U = zplanes(g_ctx, "hgevr.u", ld, n);
    const ZPlanes X = zplanes(g_ctx, "hgevr.a", ld, nrhs);
    zsplit(st, u_dev, ldu, n, n, true, U, ld);
    zsplit(st, x_dev, ldx, n, nrhs, false, X, ld);
    const ZTriInv V = ztri_inverses_dev(g_ctx, n, U, ld);
    ztrsm_upper_dev(g_ctx, trans, n, nrhs, U, ld, X, ld, V, false);
    zjoin(st, X, ld, n, nrhs, false, x_dev, ldx);
    EIGX_HIP_CHECK(hipStreamSynchronize(st));
    return EIGX_OK;
  });
}

// upper(a) <- U^-H A U^-1 for the upper triangle of a on entry; the strict lower triangle of a is left as it was
int eigx_hgev_reduce_dev(int n, double* a_dev, int lda, const double* u_dev, int ldu) {
  if (!g_ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  if (n <= 0 || !a_dev || !u_dev || lda < n || ldu < n) return EIGX_ERR_BAD_ARG;
  if (g_ctx.grid.nranks != 1) return EIGX_ERR_INTERNAL;
  return eigx_guard(g_ctx, [&] {
    EIGX_HIP_CHECK(hipSetDevice(g_ctx.device));
    EIGX_HIP_CHECK(hipStreamSynchronize(nullptr));
    hipStream_t st = g_ctx.stream;
    const int ld = pad_ld(n);
    const ZPlanes U = zplanes(g_ctx, "hgevr.u", ld, n);
    const ZPlanes A = zplanes(g_ctx, "hgevr.a", ld, n);
    const ZPlanes Cp = zplanes(g_ctx, "hgevr.cp", ld, n);
    zsplit(st, u_dev, ldu, n, n, true, U, ld);
    zexpand(st, a_dev, lda, n, A, ld);
    const ZTriInv V = ztri_inverses_dev(g_ctx, n, U, ld);
    hgev_reduce_dev(g_ctx, n, A, ld, U, ld, V, Cp, ld);
    zjoin(st, Cp, ld, n, n, true, a_dev, lda);
    EIGX_HIP_CHECK(hipStreamSynchronize(st));
    return EIGX_OK;
  });
}

}  // extern "C"
