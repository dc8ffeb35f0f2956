// hbatch_range.hip -- eigx_h_batch_range (EXTENSION, not in the reference): eigenpairs il .. iu of many small complex Hermitian
// matrices (n <= EIGX_HBATCH_NMAX) in one launch, one workgroup per matrix, the matrix resident in LDS from load to store (DESIGN
// section 8o).  The complex sibling of batch_range.hip.  The window kernel (route 1):
//   load the upper triangle (interleaved complex), mirror it with conjugation into the split planes Ar, Ai, scan for NaN / Inf,
//   scale (as hbatch_kernel, hbatch.hip)
//   -> Hermitian Householder tridiagonalisation only and the chain of unit phases (the first loop of herm_tridiag_ql: the reflectors
//      stay in the planes' columns, Q is not formed) -> a real (d, e >= 0)
//   -> the real tridiagonal window stage of batch_window.h: Sturm-count multi-section; mode 'A': inverse iteration, two passes of
//      Gram-Schmidt with the acceptance test of key 27, Rayleigh-Ritz on the m x m projection -> the real Y S
//   -> V = D (Y S) on two planes over the dead window storage, the n - 1 Hermitian reflectors applied to its m columns -> unscale,
//      store w(1:m), z(1:n, 1:m) interleaved.
// No workgroup talks to another, no atomics on the data, every sum in an order that depends on n and the window alone.  A matrix
// the acceptance test refuses leaves a mark and is solved again by route 2: eigx_h_batch_dev into pooled workspace and a gather
// of the window (bit for bit the slice of that entry's result).  n above the cutoff of eigx_h_batch (eigx_tune key 22) goes
// through herm_range_dev matrix by matrix (route 3).  Which of routes 1 and 2 a call takes: eigx_tune key 26.
// This file holds the window kernel, the measured-route table and the family's WindowFamily record; the routes, the redo and the
// gather are the windowed frame's (batch_frame.hip), the reduction is herm_tridiag (batch_tridiag.h).
#include "eigx_context.h"
#include "batch_common.h"
#include "batch_tridiag.h"
#include "batch_window.h"
#include "../../include/eigenexa_amd.h"
#include <cfloat>

#pragma clang fp contract(off)

namespace eigx {
namespace {

// One workgroup of 2 NMAX threads per matrix, thread (r, hh) = (row, half) as in hbatch_kernel.  MW: the widest window of mode 'A';
// MW = 0: an instance without window storage, which serves mode 'N' only (the class of 96, whose planes leave no room for it).
// F, Y: the window storage of batch_window.h; after the Rayleigh-Ritz step the planes Vr, Vi of the back-transformation lie over
// F's first quarter and over Y.  k0 = il - 1, m = iu - il + 1; want_vec needs m <= MW.  redo[k] = 1: the acceptance test refused
// matrix k and nothing of it was written.
template <int NMAX, int MW>
__global__ __launch_bounds__(2 * NMAX) void hbatch_range_kernel(int n, int batch, int k0, int m, const double* __restrict__ a, int lda,
                                                                int64_t stride_a, double* __restrict__ w, int ldw,
                                                                double* __restrict__ z, int ldz, int64_t stride_z, int want_vec,
                                                                double accept, int* __restrict__ info,
                                                                unsigned long long* __restrict__ first, int* __restrict__ redo) {
  constexpr int NT = 2 * NMAX, LD = NMAX + 1;
  constexpr int WN = MW > 0 ? NMAX * MW : 1, WM = MW > 0 ? MW : 1, WH = MW > 0 ? NMAX : 1;
  __shared__ double Ar[LD * NMAX], Ai[LD * NMAX];
  __shared__ double d[NMAX], e[NMAX], hv[NMAX];
  __shared__ double pr[NMAX], pi[NMAX];  // the off-diagonal entries g of the Hermitian tridiagonal matrix, then the phases
  __shared__ double ur[NMAX], ui[NMAX], qr[NMAX], qi[NMAX];
  __shared__ double pt[4 * NMAX];        // partial sums (re, im); the counts of a multi-section round; (c_i, s_i) of a QL iteration
  __shared__ double red[4][4];
  __shared__ double hs[WH];              // hv, kept across the Rayleigh-Ritz step
  __shared__ double F[4 * WN];
  __shared__ double Y[WN];
  __shared__ double lamv[WM];
  __shared__ int perm[WM];
  __shared__ int ctl[4];
  __shared__ int bad;                    // a lane of the inverse iteration met a vector without a norm
  __shared__ unsigned long long msk[2];
  const int tid = threadIdx.x, r = tid % NMAX, hh = tid / NMAX;
  const bool row = hh == 0 && r < n;

  for (int k = blockIdx.x; k < batch; k += gridDim.x) {
    // ---- 1. load the upper triangle, mirror with conjugation, scan, scale (hbatch_kernel) ------------------------------------
    const double* ak = a + 2 * (size_t)k * stride_a;
    double mx = 0.0, nf = 0.0;
    for (int j = hh; j < n; j += 2) {
      if (r <= j) {
        const size_t at = 2 * (r + (size_t)j * lda);
        const double xr = ak[at];
        const double xi = r < j ? ak[at + 1] : 0.0;   // the imaginary part of the diagonal is not read
        if (!(fabs(xr) <= DBL_MAX) || !(fabs(xi) <= DBL_MAX)) nf = 1.0;
        else mx = fmax(mx, fmax(fabs(xr), fabs(xi)));
        Ar[r + j * LD] = xr;
        Ai[r + j * LD] = xi;
        Ar[j + r * LD] = xr;
        Ai[j + r * LD] = -xi;
      }
    }
    nf = block_max<NT>(nf, red[0]);
    mx = block_max<NT>(mx, red[1]);      // (its barrier also publishes the mirrored entries)
    if (nf != 0.0) {                     // uniform
      fail_matrix(k, EIGX_ERR_NONFINITE, row && r < m, r, w, ldw, info, first);
      if (tid == 0) redo[k] = 0;
      continue;
    }
    const int ex = scale_exponent(mx, false);
    const double unscale = ldexp(1.0, ex);
    if (ex != 0) {
      const double sigma = ldexp(1.0, -ex);
      if (r < n)
        for (int j = hh; j < n; j += 2) { Ar[r + j * LD] *= sigma; Ai[r + j * LD] *= sigma; }
    }
    if (tid == 0) bad = 0;
    __syncthreads();

    // ---- 2. tridiagonalisation and phase chain only ------------------------------------------------------------------------------
    herm_tridiag<NMAX>(n, Ar, Ai, d, e, hv, pr, pi, ur, ui, qr, qi, pt, red);

    // ---- 3. the real window stage on (d, e): eigenvalues k0 .. k0 + m - 1 by multi-section (qr <- e^2) ----------------------------
    const WindowBounds tb = window_bounds<NMAX>(n, d, e, qr, red);
    if (tb.tnorm == 0.0) {               // the zero matrix (uniform): w = 0 exactly, unit vectors
      if (want_vec && !(1.0 >= accept)) {   // (their norm is 1: a bound above it refuses them like any others)
        if (tid == 0) redo[k] = 1;
        __syncthreads();
        continue;
      }
      if (tid < m) w[(size_t)k * ldw + tid] = 0.0;
      if (want_vec && r < n) {
        double* zk = z + 2 * (size_t)k * stride_z;
        for (int c = hh; c < m; c += 2) {
          const size_t at = 2 * (r + (size_t)c * ldz);
          zk[at] = r == k0 + c ? 1.0 : 0.0;
          zk[at + 1] = 0.0;
        }
      }
      if (tid == 0) {
        if (info) info[k] = 0;
        redo[k] = 0;
      }
      __syncthreads();
      continue;
    }
    {
      const double lam = window_multisection<NMAX>(n, k0, m, d, qr, (int*)pt, tb);
      const int G = NT / m < 64 ? NT / m : 64;
      if (tid / G < m && tid % G == 0) {
        if (MW > 0 && want_vec) lamv[tid / G] = lam;
        else w[(size_t)k * ldw + tid / G] = lam * unscale;
      }
    }
    if (MW == 0 || !want_vec) {          // uniform
      if (tid == 0) {
        if (info) info[k] = 0;
        redo[k] = 0;
      }
      __syncthreads();
      continue;
    }
    if constexpr (MW > 0) {
      __syncthreads();
      window_inverse_iteration<NMAX, MW>(n, m, d, e, lamv, F, Y, tb.epsT, &bad);
      if (window_gram_schmidt<NMAX, MW>(n, m, Y, pt, ur, red, accept, bad != 0)) {   // uniform: route 2 solves this matrix again
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

      // ---- 4. back-transformation: V = D (Y S), then Z = H_{n-1} ... H_1 V, the order of herm_tridiag_ql's second loop ------------
      constexpr int CH = NT / MW;
      const int wc = tid % MW, wch = tid / MW;   // thread (column, chunk of rows) of the window-wide sums
      double* Vr = F;                    // (Y S lies here: row i is multiplied by p_i in place)
      double* Vi = Y;
      for (int idx = tid; idx < n * MW; idx += NT) {
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
            const double ucr = Ar[t + i * LD], uci = Ai[t + i * LD], vr = Vr[t * MW + wc], vi = Vi[t * MW + wc];
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
          const double vr = Ar[r + i * LD], vi = Ai[r + i * LD];
          for (int c = hh; c < m; c += 2) {
            const double scr = qr[c], sci = qi[c];
            Vr[r * MW + c] = fma(sci, vi, fma(-scr, vr, Vr[r * MW + c]));
            Vi[r * MW + c] = fma(-sci, vr, fma(-scr, vi, Vi[r * MW + c]));
          }
        }
        __syncthreads();
      }
      if (tid < m) w[(size_t)k * ldw + tid] = lamv[tid] * unscale;
      if (r < n) {
        double* zk = z + 2 * (size_t)k * stride_z;
        for (int c = hh; c < m; c += 2) {
          const size_t at = 2 * (r + (size_t)c * ldz);
          zk[at] = Vr[r * MW + c];
          zk[at + 1] = Vi[r * MW + c];
        }
      }
      if (tid == 0) {
        if (info) info[k] = 0;
        redo[k] = 0;
      }
      __syncthreads();
    }
  }
}

// the widest window the class of n serves in mode 'A' (0: the class has no window storage)
int hwindow_width(int n) { return n <= 64 ? 16 : 0; }

// The automatic rule of key 26 = 0 for this family, read off the table of DESIGN section 8o (profiles/hbatch_range_time.log):
// route 1 only where it measured faster than route 2 by more than the spread of the repeats; a cell that is not measured takes
// route 2.  Measured at n = 8, 16, 32, 64 with m = 1, 4, 16 (mode 'N' also m = n) and at n = 96 in mode 'N'; a size takes the row
// of the largest measured size not above it, a width the row of the smallest measured width not below it (the rule of section 8n).
//   n < 16        route 2 (n = 8: route 1 took 1.4 to 3.7 times as long)
//   16 <= n < 32  'A': route 2 (m = 1: 0.96, m = 4: 0.80)        'N': m <= 4 (1.05; m = 16: 0.87)
//   32 <= n < 64  'A': m <= 4 (1.30; m = 16: 0.63)               'N': every m (1.12 at m = 32)
//   n >= 64       every eligible cell (1.49 to 5.9)
bool hroute1_measured_faster(int n, char mode, int m) {
  if (n < 16) return false;
  if (n < 32) return mode == 'N' && m <= 4;
  if (n < 64) return mode == 'A' ? m <= 4 : true;
  return true;
}

void hbrange_launch(const BatchArgs& g, int k0, int m, double accept, hipStream_t st, unsigned long long* first, int* redo) {
  with_n_class<EIGX_HBATCH_NMAX>(g.n, [&](auto nmax) {
    constexpr int NMAX = decltype(nmax)::value;
    constexpr int MW = NMAX <= 64 ? 16 : 0;
    hipLaunchKernelGGL((hbatch_range_kernel<NMAX, MW>), dim3((unsigned)g.batch), dim3(2 * NMAX), 0, st, g.n, g.batch, k0, m,
                       (const double*)g.a, g.lda, g.stride_a, g.w, g.ldw, g.z, g.ldz, g.stride_z, (int)(g.mode == 'A'), accept, g.info,
                       first, redo);
  });
}

int hbrange_full_solve(const BatchArgs& c) {
  return eigx_h_batch_dev(c.n, c.batch, c.a, c.lda, c.stride_a, c.w, c.ldw, c.z, c.ldz, c.stride_z, c.mode, c.info);
}

// route 3: eigx_h_range_dev with the interface's default block sizes on matrix k
int hbrange_solve_window(Context& ctx, const BatchArgs& g, int k, int il, int iu) {
  return herm_range_dev(ctx, g.n, RangeWindow::index(il, iu), g.block(g.a, g.stride_a, k), g.lda, g.w + (size_t)k * g.ldw,
                        g.mode == 'A' ? g.block(g.z, g.stride_z, k) : nullptr, g.ldz, 48, 128, g.mode);
}

// (the pool names are part of the description of the entry in include/eigenexa_amd_hbatch_range.h)
const WindowFamily hbrange_family{get_hbatch_nmax, hwindow_width, hroute1_measured_faster, hbrange_launch, hbrange_full_solve,
                                  hbrange_solve_window, "hbrange.first", "hbrange.redo", "hbatch.rw", "hbatch.rz", "hbatch.rinfo",
                                  {"hbrange.ha", nullptr, "hbrange.hz", "hbrange.hw", "hbrange.hinfo"}};

}  // namespace
}  // namespace eigx

using namespace eigx;

extern "C" {

// EXTENSION: eigenpairs il .. iu of `batch` complex Hermitian matrices of one size (one GPU; a, z interleaved complex, lda, ldz
// and the strides in elements); see brange_frame_host / brange_frame_dev (batch_frame.hip)
int eigx_h_batch_range(int n, int batch, int il, int iu, double* a, int lda, int64_t stride_a, double* w, int ldw, double* z, int ldz,
                       int64_t stride_z, char mode, int* info) {
  const BatchArgs g{n, batch, a, lda, stride_a, nullptr, 0, 0, w, ldw, z, ldz, stride_z, mode, info, 16, false};
  return eigx_guard(g_ctx, [&] { return brange_frame_host(g_ctx, g, il, iu, hbrange_family); });
}
int eigx_h_batch_range_dev(int n, int batch, int il, int iu, double* a_dev, int lda, int64_t stride_a, double* w_dev, int ldw,
                           double* z_dev, int ldz, int64_t stride_z, char mode, int* info_dev) {
  const BatchArgs g{n, batch, a_dev, lda, stride_a, nullptr, 0, 0, w_dev, ldw, z_dev, ldz, stride_z, mode, info_dev, 16, false};
  return eigx_guard(g_ctx, [&] { return brange_frame_dev(g_ctx, g, il, iu, hbrange_family); });
}

}  // extern "C"
