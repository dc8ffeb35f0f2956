// hgbatch_range.hip -- eigx_hgev_batch_range (EXTENSION, not in the reference): eigenpairs il .. iu of many small Hermitian-definite
// pencils A x = lambda B x (n <= EIGX_HGBATCH_NMAX) in one launch, one workgroup per pencil, the four split planes of both matrices
// resident in LDS from load to store.  The complex sibling of gbatch_range.hip.  The window kernel (route 1):
//   load the upper triangles of A (mirrored with conjugation) and B (interleaved complex), scan, scale, B = U^H U,
//   C = U^-H A U^-1, mirror, scan, scale: phases 1 to 3 of hgbatch_kernel (hgbatch.hip), the same arithmetic in the same order, so
//   U is bit for bit that entry's
//   -> Hermitian Householder tridiagonalisation of C only and the chain of unit phases (herm_tridiag of batch_tridiag.h: the
//      reflectors stay in the planes' columns, Q is not formed) -> a real (d, e >= 0)
//   -> the real tridiagonal window stage of batch_window.h: Sturm-count multi-section; mode 'A': inverse iteration, two passes of
//      Gram-Schmidt with the acceptance test of key 27, Rayleigh-Ritz on the m x m projection -> the real Y S
//   -> V = D (Y S) on two planes over the dead window storage, the n - 1 Hermitian reflectors applied to its m columns (step 4 of
//      hbatch_range_kernel) -> Z = U^-1 V by a backward substitution on the m columns (step 5 of gbatch_range_kernel over complex
//      numbers) -> unscale, store w(1:m), z(1:n, 1:m) interleaved and U (into b).
// No workgroup talks to another, no atomics on the data, every sum in an order that depends on n and the window alone.  A pencil
// the acceptance test refuses leaves a mark, writes nothing (b included) and is solved again by route 2: eigx_hgev_batch_dev on the
// caller's a and b (so U lands in b) with w and z in pooled workspace, and a gather of the window (bit for bit the slice of that
// entry's result).  n above the cutoff of eigx_hgev_batch (eigx_tune key 24) goes through hgev_range_dev pencil by pencil
// (route 3).  Which of routes 1 and 2 a call takes: eigx_tune key 26.
// This file holds the window kernel, the measured-route table and the family's WindowFamily record; the routes, the redo and the
// gather are the windowed frame's (batch_frame.hip), the reduction is herm_tridiag (batch_tridiag.h).
#include "eigx_context.h"
#include "batch_common.h"
#include "batch_solve.h"
#include "batch_tridiag.h"
#include "batch_window.h"
#include "../../include/eigenexa_amd.h"
#include <cfloat>

#pragma clang fp contract(off)

namespace eigx {
namespace {

// The shared arrays of an instance, added up (bytes): four planes, nine vectors of NMAX doubles, pt, red, hs, F, Y and the small
// control words (lamv, perm, ctl, ibad, msk).  The compiler's own figure is in DESIGN section 8q.
constexpr size_t hgbatch_range_lds(int NMAX, int MW) {
  return (size_t)8 * (4 * (NMAX + 1) * NMAX + 9 * NMAX + 4 * NMAX + 16 + NMAX + 4 * NMAX * MW + NMAX * MW + MW) + 4 * MW + 16 + 4 + 16;
}

// One workgroup of 2 NMAX threads per pencil, thread (r, hh) = (row, half) as in hgbatch_kernel.  The split planes Sr, Si(LD, NMAX)
// hold A, then C, then the reflectors of its reduction; Ur, Ui(LD, NMAX) hold B, then its factor (upper triangle; the strict lower
// triangle is never read, the imaginary part of the diagonal never computed).  MW: the widest window of mode 'A' (16 in the class
// of 32, 8 in the class of 64, whose planes alone take 133 120 of the 163 840 bytes).  F, Y: the window storage of batch_window.h;
// after the Rayleigh-Ritz step the planes Vr, Vi of V = D (Y S), entry (i, c) at [i MW + c], lie over F's first quarter and over Y
// and stay there through steps 4 and 5.  k0 = il - 1, m = iu - il + 1; want_vec needs m <= MW.  redo[k] = 1: the acceptance test
// refused pencil k and nothing of it was written, b included.
template <int NMAX, int MW>
__global__ __launch_bounds__(2 * NMAX) void hgbatch_range_kernel(int n, int batch, int k0, int m, const double* __restrict__ a, int lda,
                                                                 int64_t stride_a, double* __restrict__ b, int ldb, int64_t stride_b,
                                                                 double* __restrict__ w, int ldw, double* __restrict__ z, int ldz,
                                                                 int64_t stride_z, int want_vec, double accept,
                                                                 int* __restrict__ info, unsigned long long* __restrict__ first,
                                                                 int* __restrict__ redo) {
  constexpr int NT = 2 * NMAX, LD = NMAX + 1;
  static_assert(MW > 0 && NT % MW == 0, "every class carries window storage");
  static_assert(hgbatch_range_lds(NMAX, MW) <= 163840, "the shared arrays exceed the LDS of a gfx950 workgroup");
  __shared__ double Sr[LD * NMAX], Si[LD * NMAX];
  __shared__ double Ur[LD * NMAX], Ui[LD * NMAX];
  __shared__ double d[NMAX], e[NMAX], hv[NMAX];
  __shared__ double pr[NMAX], pi[NMAX];  // the off-diagonal entries g of the Hermitian tridiagonal matrix, then the phases
  __shared__ double ur[NMAX], ui[NMAX], qr[NMAX], qi[NMAX];
  __shared__ double pt[4 * NMAX];        // partial sums (re, im); the counts of a multi-section round; (c_i, s_i) of a QL iteration
  __shared__ double red[4][4];
  __shared__ double hs[NMAX];            // hv, kept across the Rayleigh-Ritz step
  __shared__ double F[4 * NMAX * MW];
  __shared__ double Y[NMAX * MW];
  __shared__ double lamv[MW];
  __shared__ int perm[MW];
  __shared__ int ctl[4];
  __shared__ int ibad;                   // a lane of the inverse iteration met a vector without a norm
  __shared__ unsigned long long msk[2];
  const int tid = threadIdx.x, r = tid % NMAX, hh = tid / NMAX;
  const bool row = hh == 0 && r < n;
  const bool wrow = row && r < m;        // the threads that own an entry of w(1:m)

  for (int k = blockIdx.x; k < batch; k += gridDim.x) {
    // ---- 1. phases 1 to 3 of hgbatch_kernel: load both upper triangles, mirror A with conjugation, scan, scale -----------------
    const double* ak = a + 2 * (size_t)k * stride_a;
    double* bk = b + 2 * (size_t)k * stride_b;
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
    mxb = block_max<NT>(mxb, red[2]);    // (the barriers also publish the loaded entries)
    if (bad != 0.0) {                    // uniform; b is as it was passed
      fail_matrix(k, EIGX_ERR_NONFINITE, wrow, r, w, ldw, info, first);
      if (tid == 0) redo[k] = 0;
      continue;
    }
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
    if (tid == 0) ibad = 0;
    __syncthreads();

    //      B = U^H U, right-looking: two barriers per column
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
    if (!spd) {
      fail_matrix(k, EIGX_ERR_NOT_SPD, wrow, r, w, ldw, info, first);
      if (tid == 0) redo[k] = 0;
      continue;
    }

    //      C = U^-H A U^-1: X = U^-H A down the columns (lane = column), C = X U^-1 along the rows (lane = row)
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
    if (bad != 0.0) {                    // uniform: B was too close to singular for C to be formed
      fail_matrix(k, EIGX_ERR_NOT_SPD, wrow, r, w, ldw, info, first);
      if (tid == 0) redo[k] = 0;
      continue;
    }
    const int exc = scale_exponent(mxc, false);
    if (exc != 0 && r < n) {
      const double sigma = ldexp(1.0, -exc);
      for (int j = hh; j < n; j += 2) { Sr[r + j * LD] *= sigma; Si[r + j * LD] *= sigma; }
    }
    __syncthreads();
    const int exw = exa - exb + exc;     // C = 2^(exb - exa - exc) times the matrix that is solved

    // ---- 2. tridiagonalisation and phase chain only ------------------------------------------------------------------------------
    herm_tridiag<NMAX>(n, Sr, Si, d, e, hv, pr, pi, ur, ui, qr, qi, pt, red);

    // ---- 3. the real window stage on (d, e): eigenvalues k0 .. k0 + m - 1 by multi-section (qr <- e^2) ----------------------------
    const WindowBounds tb = window_bounds<NMAX>(n, d, e, qr, red);
    const bool zero = tb.tnorm == 0.0;   // the zero C (uniform): w = 0 exactly, the unit vectors k0 .. k0 + m - 1 through step 5
    const bool vec = want_vec != 0;
    double* Vr = F;
    double* Vi = Y;
    if (zero) {
      if (vec && !(1.0 >= accept)) {     // (their norm is 1: a bound above it refuses them like any others)
        if (tid == 0) redo[k] = 1;
        __syncthreads();
        continue;
      }
      if (vec) {
        if (tid < m) lamv[tid] = 0.0;
        for (int idx = tid; idx < n * MW; idx += NT) {
          Vr[idx] = idx / MW == k0 + idx % MW ? 1.0 : 0.0;
          Vi[idx] = 0.0;
        }
      } else if (tid < m) {
        w[(size_t)k * ldw + tid] = 0.0;
      }
    } else {
      const double lam = window_multisection<NMAX>(n, k0, m, d, qr, (int*)pt, tb);
      const int G = NT / m < 64 ? NT / m : 64;
      if (tid / G < m && tid % G == 0) {
        if (vec) lamv[tid / G] = lam;
        else w[(size_t)k * ldw + tid / G] = ldexp(lam, exw);
      }
    }
    if (!vec) {                          // uniform: the eigenvalues are stored; U goes into b
      if (r < n)
        for (int j = hh; j < n; j += 2)
          if (r <= j) {
            const size_t at = 2 * (r + (size_t)j * ldb);
            bk[at] = ldexp(Ur[r + j * LD], exb / 2);
            bk[at + 1] = r < j ? ldexp(Ui[r + j * LD], exb / 2) : 0.0;
          }
      if (tid == 0) {
        if (info) info[k] = 0;
        redo[k] = 0;
      }
      __syncthreads();
      continue;
    }
    __syncthreads();
    if (!zero) {                         // uniform
      window_inverse_iteration<NMAX, MW>(n, m, d, e, lamv, F, Y, tb.epsT, &ibad);
      if (window_gram_schmidt<NMAX, MW>(n, m, Y, pt, ur, red, accept, ibad != 0)) {   // uniform: route 2 solves this pencil again
        if (tid == 0) redo[k] = 1;
        __syncthreads();
        continue;
      }
      if (row) hs[r] = hv[r];
      if (!window_rayleigh_ritz<NMAX, MW>(n, m, d, e, hv, ur, qr, pt, red, ctl, msk, F, Y, lamv, perm)) {   // uniform
        if (tid == 0) redo[k] = 1;
        __syncthreads();
        continue;
      }

      // ---- 4. back-transformation: V = D (Y S), then V <- H_{n-1} ... H_1 V, step 4 of hbatch_range_kernel in the same order ------
      constexpr int CH = NT / MW;
      const int wc = tid % MW, wch = tid / MW;   // thread (column, chunk of rows) of the window-wide sums
      for (int idx = tid; idx < n * MW; idx += NT) {   // (Y S lies in Vr: row i is multiplied by p_i in place)
        const int i = idx / MW, c = idx % MW;
        if (c < m) {
          const double x = Vr[idx];
          Vr[idx] = pr[i] * x;
          Vi[idx] = pi[i] * x;
        }
      }
      __syncthreads();
      for (int i = 1; i < n; ++i) {
        const double h = hs[i];
        if (h == 0.0) continue;          // uniform
        const int l = i - 1;
        double sr = 0.0, si = 0.0;       // s = u^H V(0 .. l, c)
        if (wc < m)
          for (int t = wch; t <= l; t += CH) {
            const double ucr = Sr[t + i * LD], uci = Si[t + i * LD], vr = Vr[t * MW + wc], vi = Vi[t * MW + wc];
            sr = fma(ucr, vr, sr);
            sr = fma(uci, vi, sr);
            si = fma(ucr, vi, si);
            si = fma(-uci, vr, si);
          }
        pt[tid] = sr;
        pt[NT + tid] = si;
        __syncthreads();
        if (tid < m) {
          double s0 = pt[tid], s1 = pt[NT + tid];
          for (int c = 1; c < CH; ++c) {
            s0 += pt[c * MW + tid];
            s1 += pt[NT + c * MW + tid];
          }
          qr[tid] = s0 / h;
          qi[tid] = s1 / h;
        }
        __syncthreads();
        if (r <= l) {                    // V(r, c) -= u_r s_c
          const double vr = Sr[r + i * LD], vi = Si[r + i * LD];
          for (int c = hh; c < m; c += 2) {
            const double scr = qr[c], sci = qi[c];
            Vr[r * MW + c] = fma(sci, vi, fma(-scr, vr, Vr[r * MW + c]));
            Vi[r * MW + c] = fma(-sci, vr, fma(-scr, vi, Vi[r * MW + c]));
          }
        }
        __syncthreads();
      }
    }

    // ---- 5. Z = U^-1 V on the m columns: a backward substitution, column-oriented.  Thread (r, hh) owns the entries of row r in
    //         the columns c = hh, hh + 2, ...; at step i the owners of row i divide it by the real U(i, i), and behind one barrier
    //         every row above takes its multiple of it: x_r = (v_r - U(r, n-1) x_{n-1} - ... - U(r, r+1) x_{r+1}) / U(r, r), the
    //         terms taken one by one in that order, whatever m and the position in the batch ---------------------------------------
    for (int i = n - 1; i >= 0; --i) {
      if (r == i) {
        const double dk = Ur[i + i * LD];
        for (int c = hh; c < m; c += 2) {
          Vr[i * MW + c] = Vr[i * MW + c] / dk;
          Vi[i * MW + c] = Vi[i * MW + c] / dk;
        }
      }
      __syncthreads();
      if (r < i) {
        const double ar = Ur[r + i * LD], ai = Ui[r + i * LD];
        for (int c = hh; c < m; c += 2) {
          const double xr = Vr[i * MW + c], xi = Vi[i * MW + c];
          Vr[r * MW + c] = fma(ai, xi, fma(-ar, xr, Vr[r * MW + c]));
          Vi[r * MW + c] = fma(-ai, xr, fma(-ar, xi, Vi[r * MW + c]));
        }
      }
    }
    __syncthreads();
    if (tid < m) w[(size_t)k * ldw + tid] = ldexp(lamv[tid], exw);
    if (r < n) {
      double* zk = z + 2 * (size_t)k * stride_z;
      for (int c = hh; c < m; c += 2) {
        const size_t at = 2 * (r + (size_t)c * ldz);
        zk[at] = ldexp(Vr[r * MW + c], -(exb / 2));
        zk[at + 1] = ldexp(Vi[r * MW + c], -(exb / 2));
      }
      for (int j = hh; j < n; j += 2)
        if (r <= j) {
          const size_t at = 2 * (r + (size_t)j * ldb);
          bk[at] = ldexp(Ur[r + j * LD], exb / 2);
          bk[at + 1] = r < j ? ldexp(Ui[r + j * LD], exb / 2) : 0.0;
        }
    }
    if (tid == 0) {
      if (info) info[k] = 0;
      redo[k] = 0;
    }
    __syncthreads();
  }
}

// the widest window the class of n serves in mode 'A': the class of 64 has room for 8 columns beside its four planes
int hgwindow_width(int n) { return n <= 32 ? 16 : 8; }

// The automatic rule of key 26 = 0 for this family, read off the table of DESIGN section 8q (profiles/hgbatch_range_time.log):
// route 1 only where it measured faster than route 2 by more than the spread of the repeats; a cell that is not measured takes
// route 2.  Measured at n = 8, 16, 32 with m = 1, 4, 16 and at n = 48, 64 with m = 1, 4, 8 (mode 'N' also m = n); a size takes the
// row of the largest measured size not above it, a width the row of the smallest measured width not below it (the rule of
// section 8n); a width above the widest measured one of its row is not measured.  Route 2 / route 1:
//   n < 32        route 2 (n = 8: 0.31 to 0.65; n = 16: 'A' 0.85 / 0.73 / 0.31, 'N' 0.88 / 0.89 / 0.75)
//   32 <= n < 48  'A': m = 1 (1.13; m = 4: 1.01, inside the spread of route 2's repeats; m = 16: 0.57)
//                 'N': m <= 16 (1.18 / 1.15 / 1.01; m = 32: 0.90)
//   48 <= n < 64  'A': every eligible m (2.55 / 2.34 / 2.04)      'N': m <= 48 (2.44 / 2.39 / 2.33 / 1.87)
//   n >= 64       every eligible cell (2.05 to 2.76)
bool hgroute1_measured_faster(int n, char mode, int m) {
  if (n < 32) return false;
  if (n < 48) return mode == 'A' ? m <= 1 : m <= 16;
  if (n < 64) return mode == 'A' ? true : m <= 48;
  return true;
}

void hgbrange_launch(const BatchArgs& g, int k0, int m, double accept, hipStream_t st, unsigned long long* first, int* redo) {
  const auto go = [&](auto nmax, auto mw) {
    constexpr int NMAX = decltype(nmax)::value, MW = decltype(mw)::value;
    hipLaunchKernelGGL((hgbatch_range_kernel<NMAX, MW>), dim3((unsigned)g.batch), dim3(2 * NMAX), 0, st, g.n, g.batch, k0, m,
                       (const double*)g.a, g.lda, g.stride_a, g.b, g.ldb, g.stride_b, g.w, g.ldw, g.z, g.ldz, g.stride_z,
                       (int)(g.mode == 'A'), accept, g.info, first, redo);
  };
  if (g.n <= 32) go(std::integral_constant<int, 32>(), std::integral_constant<int, 16>());
  else go(std::integral_constant<int, EIGX_HGBATCH_NMAX>(), std::integral_constant<int, 8>());
}

int hgbrange_full_solve(const BatchArgs& c) {
  return eigx_hgev_batch_dev(c.n, c.batch, c.a, c.lda, c.stride_a, c.b, c.ldb, c.stride_b, c.w, c.ldw, c.z, c.ldz, c.stride_z, c.mode,
                             c.info);
}

// route 3: eigx_hgev_range_dev on pencil k, which takes every leading dimension >= n: nothing is staged
int hgbrange_solve_window(Context& ctx, const BatchArgs& g, int k, int il, int iu) {
  return hgev_range_dev(ctx, g.n, RangeWindow::index(il, iu), g.block(g.a, g.stride_a, k), g.lda, g.block(g.b, g.stride_b, k), g.ldb,
                        g.w + (size_t)k * g.ldw, g.mode == 'A' ? g.block(g.z, g.stride_z, k) : nullptr, g.ldz, g.mode);
}

// (the pool names are part of the description of the entry in include/eigenexa_amd_hgbatch_range.h)
const WindowFamily hgbrange_family{get_hgbatch_nmax, hgwindow_width, hgroute1_measured_faster, hgbrange_launch, hgbrange_full_solve,
                                   hgbrange_solve_window, "hgbrange.first", "hgbrange.redo", "hgbrange.rw", "hgbrange.rz",
                                   "hgbrange.rinfo", {"hgbrange.ha", "hgbrange.hb", "hgbrange.hz", "hgbrange.hw", "hgbrange.hinfo"}};

}  // namespace
}  // namespace eigx

using namespace eigx;

extern "C" {

// EXTENSION: eigenpairs il .. iu of `batch` Hermitian-definite pencils of one size (one GPU; a, b, z interleaved complex, lda, ldb,
// ldz and the strides in complex elements); see brange_frame_host / brange_frame_dev (batch_frame.hip)
int eigx_hgev_batch_range(int n, int batch, int il, int iu, double* a, int lda, int64_t stride_a, double* b, int ldb, int64_t stride_b,
                          double* w, int ldw, double* z, int ldz, int64_t stride_z, char mode, int* info) {
  const BatchArgs g{n, batch, a, lda, stride_a, b, ldb, stride_b, w, ldw, z, ldz, stride_z, mode, info, 16, true};
  return eigx_guard(g_ctx, [&] { return brange_frame_host(g_ctx, g, il, iu, hgbrange_family); });
}
int eigx_hgev_batch_range_dev(int n, int batch, int il, int iu, double* a_dev, int lda, int64_t stride_a, double* b_dev, int ldb,
                              int64_t stride_b, double* w_dev, int ldw, double* z_dev, int ldz, int64_t stride_z, char mode,
                              int* info_dev) {
  const BatchArgs g{n, batch, a_dev, lda, stride_a, b_dev, ldb, stride_b, w_dev, ldw, z_dev, ldz, stride_z, mode, info_dev, 16, true};
  return eigx_guard(g_ctx, [&] { return brange_frame_dev(g_ctx, g, il, iu, hgbrange_family); });
}

}  // extern "C"
