// gbatch_range.hip -- eigx_gev_batch_range (EXTENSION, not in the reference): eigenpairs il .. iu of many small symmetric-definite
// pencils A x = lambda B x (n <= EIGX_GBATCH_NMAX) in one launch, one workgroup per pencil, both matrices resident in LDS from
// load to store.  The pencil sibling of batch_range.hip.  The window kernel (route 1):
//   load the upper triangles of A (mirrored) and B, scan, scale, B = U^T U, C = U^-T A U^-1, mirror, scan, scale: phases 1 to 3 of
//   gbatch_kernel (gbatch.hip), the same arithmetic in the same order, so U is bit for bit that entry's
//   -> Householder tridiagonalisation of C only (sym_tridiag of batch_tridiag.h: the reflectors stay in S's columns, Q is not formed)
//   -> the real tridiagonal window stage of batch_window.h: Sturm-count multi-section; mode 'A': inverse iteration, two passes of
//      Gram-Schmidt with the acceptance test of key 27, Rayleigh-Ritz on the m x m projection -> Y S
//   -> the n - 1 reflectors applied to its m columns (step 7 of batch_range_kernel) -> Z = U^-1 V by a backward substitution on
//      the m columns -> unscale, store w(1:m), z(1:n, 1:m) and U (into b).
// No workgroup talks to another, no atomics on the data, every sum in an order that depends on n and the window alone.  A pencil
// the acceptance test refuses leaves a mark, writes nothing (b included) and is solved again by route 2: eigx_gev_batch_dev on the
// caller's a and b (so U lands in b) with w and z in pooled workspace, and a gather of the window (bit for bit the slice of that
// entry's result).  n above the cutoff of eigx_gev_batch (eigx_tune key 23) goes through gev_range_dev pencil by pencil
// (route 3).  Which of routes 1 and 2 a call takes: eigx_tune key 26.
// This file holds the window kernel, the measured-route table and the family's WindowFamily record; the routes, the redo and the
// gather are the windowed frame's (batch_frame.hip), the reduction is sym_tridiag (batch_tridiag.h).
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

// One workgroup of 2 NMAX threads per pencil, thread (r, hh) = (row, half) as in gbatch_kernel.  S(LD, NMAX) holds A, then C, then
// the reflectors of its reduction; U(LD, NMAX) holds B, then its factor (upper triangle; the strict lower triangle is never
// read).  MW: the widest window of mode 'A'; MW = 0: an instance without window storage, which serves mode 'N' only (the class of
// 96, whose two matrices leave no room for it).  F, Y: the window storage of batch_window.h; after the Rayleigh-Ritz step V = Y S,
// entry (i, c) at [i MW + c], lies in F's first quarter and stays there through steps 4 and 5.  k0 = il - 1, m = iu - il + 1;
// want_vec needs m <= MW.  redo[k] = 1: the acceptance test refused pencil k and nothing of it was written, b included.
template <int NMAX, int MW>
__global__ __launch_bounds__(2 * NMAX) void gbatch_range_kernel(int n, int batch, int k0, int m, const double* __restrict__ a, int lda,
                                                                int64_t stride_a, double* __restrict__ b, int ldb, int64_t stride_b,
                                                                double* __restrict__ w, int ldw, double* __restrict__ z, int ldz,
                                                                int64_t stride_z, int want_vec, double accept,
                                                                int* __restrict__ info, unsigned long long* __restrict__ first,
                                                                int* __restrict__ redo) {
  constexpr int NT = 2 * NMAX, LD = NMAX + 1;
  constexpr int WN = MW > 0 ? NMAX * MW : 1, WM = MW > 0 ? MW : 1, WH = MW > 0 ? NMAX : 1;
  __shared__ double S[LD * NMAX];
  __shared__ double U[LD * NMAX];
  __shared__ double d[NMAX], e[NMAX], hv[NMAX], u[NMAX], q[NMAX];
  __shared__ double pt[2 * NMAX];        // partial sums; the counts of a multi-section round; (c_i, s_i) of a QL iteration
  __shared__ double red[4][4];
  __shared__ double hs[WH];              // hv, kept across the Rayleigh-Ritz step
  __shared__ double F[4 * WN];
  __shared__ double Y[WN];
  __shared__ double lamv[WM];
  __shared__ int perm[WM];
  __shared__ int ctl[4];
  __shared__ int ibad;                   // a lane of the inverse iteration met a vector without a norm
  __shared__ unsigned long long msk[2];
  const int tid = threadIdx.x, r = tid % NMAX, hh = tid / NMAX;
  const bool row = hh == 0 && r < n;
  const bool wrow = row && r < m;        // the threads that own an entry of w(1:m)

  for (int k = blockIdx.x; k < batch; k += gridDim.x) {
    // ---- 1. phases 1 to 3 of gbatch_kernel: load both upper triangles, mirror A, scan, scale ------------------------------------
    const double* ak = a + (size_t)k * stride_a;
    double* bk = b + (size_t)k * stride_b;
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
      for (int j = hh; j < n; j += 2) S[r + j * LD] *= sigma;
    }
    if (exb != 0 && r < n) {
      const double sigma = ldexp(1.0, -exb);
      for (int j = hh; j < n; j += 2)
        if (r <= j) U[r + j * LD] *= sigma;
    }
    if (tid == 0) ibad = 0;
    __syncthreads();

    //      B = U^T U, right-looking: two barriers per column
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
    if (!spd) {
      fail_matrix(k, EIGX_ERR_NOT_SPD, wrow, r, w, ldw, info, first);
      if (tid == 0) redo[k] = 0;
      continue;
    }

    //      C = U^-T A U^-1: X = U^-T A down the columns (lane = column), C = X U^-1 along the rows (lane = row)
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
    if (bad != 0.0) {                    // uniform: B was too close to singular for C to be formed
      fail_matrix(k, EIGX_ERR_NOT_SPD, wrow, r, w, ldw, info, first);
      if (tid == 0) redo[k] = 0;
      continue;
    }
    const int exc = scale_exponent(mxc, false);
    if (exc != 0 && r < n) {
      const double sigma = ldexp(1.0, -exc);
      for (int j = hh; j < n; j += 2) S[r + j * LD] *= sigma;
    }
    __syncthreads();
    const int exw = exa - exb + exc;     // C = 2^(exb - exa - exc) times the matrix that is solved

    // ---- 2. tridiagonalisation only ---------------------------------------------------------------------------------------------
    sym_tridiag<NMAX>(n, S, d, e, hv, u, q, pt, red);

    // ---- 3. the real window stage on (d, e): eigenvalues k0 .. k0 + m - 1 by multi-section (q <- e^2) -----------------------------
    const WindowBounds tb = window_bounds<NMAX>(n, d, e, q, red);
    const bool zero = tb.tnorm == 0.0;   // the zero C (uniform): w = 0 exactly, the unit vectors k0 .. k0 + m - 1 through step 5
    const bool vec = MW > 0 && want_vec;
    if (zero) {
      if (vec && !(1.0 >= accept)) {     // (their norm is 1: a bound above it refuses them like any others)
        if (tid == 0) redo[k] = 1;
        __syncthreads();
        continue;
      }
      if (vec) {
        if (tid < m) lamv[tid] = 0.0;
        for (int idx = tid; idx < n * WM; idx += NT) F[idx] = idx / WM == k0 + idx % WM ? 1.0 : 0.0;
      } else if (tid < m) {
        w[(size_t)k * ldw + tid] = 0.0;
      }
    } else {
      const double lam = window_multisection<NMAX>(n, k0, m, d, q, (int*)pt, tb);
      const int G = NT / m < 64 ? NT / m : 64;
      if (tid / G < m && tid % G == 0) {
        if (vec) lamv[tid / G] = lam;
        else w[(size_t)k * ldw + tid / G] = ldexp(lam, exw);
      }
    }
    if (!vec) {                          // uniform: the eigenvalues are stored; U goes into b
      if (r < n)
        for (int j = hh; j < n; j += 2)
          if (r <= j) bk[r + (size_t)j * ldb] = ldexp(U[r + j * LD], exb / 2);
      if (tid == 0) {
        if (info) info[k] = 0;
        redo[k] = 0;
      }
      __syncthreads();
      continue;
    }
    if constexpr (MW > 0) {
      __syncthreads();
      double* V = F;
      if (!zero) {                       // uniform
        window_inverse_iteration<NMAX, MW>(n, m, d, e, lamv, F, Y, tb.epsT, &ibad);
        if (window_gram_schmidt<NMAX, MW>(n, m, Y, pt, u, red, accept, ibad != 0)) {   // uniform: route 2 solves this pencil again
          if (tid == 0) redo[k] = 1;
          __syncthreads();
          continue;
        }
        if (row) hs[r] = hv[r];
        if (!window_rayleigh_ritz<NMAX, MW>(n, m, d, e, hv, u, q, pt, red, ctl, msk, F, Y, lamv, perm)) {   // uniform
          if (tid == 0) redo[k] = 1;
          __syncthreads();
          continue;
        }

        // ---- 4. back-transformation: V = H_{n-1} ... H_1 (Y S), step 7 of batch_range_kernel in the same order --------------------
        constexpr int CH = NT / MW;
        const int wc = tid % MW, wch = tid / MW;   // thread (column, chunk of rows) of the window-wide sums
        for (int i = 1; i < n; ++i) {
          const double h = hs[i];
          if (h == 0.0) continue;        // uniform
          const int l = i - 1;
          double acc = 0.0;
          if (wc < m)
            for (int t = wch; t <= l; t += CH) acc = fma(S[t + i * LD], V[t * MW + wc], acc);
          pt[tid] = acc;
          __syncthreads();
          if (tid < m) {
            double s = pt[tid];
            for (int c = 1; c < CH; ++c) s += pt[c * MW + tid];
            u[tid] = s / h;
          }
          __syncthreads();
          if (r <= l) {
            const double ur = S[r + i * LD];
            for (int c = hh; c < m; c += 2) V[r * MW + c] = fma(-u[c], ur, V[r * MW + c]);
          }
          __syncthreads();
        }
      }

      // ---- 5. Z = U^-1 V on the m columns: a backward substitution, column-oriented.  Thread (r, hh) owns the entries of row r
      //         in the columns c = hh, hh + 2, ...; at step i the owners of row i divide it by U(i, i), and behind one barrier
      //         every row above takes its multiple of it: x_r = (v_r - U(r, n-1) x_{n-1} - ... - U(r, r+1) x_{r+1}) / U(r, r), the
      //         terms taken one by one in that order, whatever m and the position in the batch ---------------------------------
      for (int i = n - 1; i >= 0; --i) {
        if (r == i) {
          const double dk = U[i + i * LD];
          for (int c = hh; c < m; c += 2) V[i * MW + c] = V[i * MW + c] / dk;
        }
        __syncthreads();
        if (r < i) {
          const double uri = U[r + i * LD];
          for (int c = hh; c < m; c += 2) V[r * MW + c] = fma(-uri, V[i * MW + c], V[r * MW + c]);
        }
      }
      __syncthreads();
      if (tid < m) w[(size_t)k * ldw + tid] = ldexp(lamv[tid], exw);
      if (r < n) {
        double* zk = z + (size_t)k * stride_z;
        for (int c = hh; c < m; c += 2) zk[r + (size_t)c * ldz] = ldexp(V[r * MW + c], -(exb / 2));
        for (int j = hh; j < n; j += 2)
          if (r <= j) bk[r + (size_t)j * ldb] = ldexp(U[r + j * LD], exb / 2);
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
int gwindow_width(int n) { return n <= 64 ? 16 : 0; }

// The automatic rule of key 26 = 0 for this family, read off the table of DESIGN section 8p (profiles/gbatch_range_time.log):
// route 1 only where it measured faster than route 2 by more than the spread of the repeats; a cell that is not measured takes
// route 2.  Measured at n = 8, 16, 32, 64 with m = 1, 4, 16 (mode 'N' also m = n) and at n = 96 in mode 'N'; a size takes the row
// of the largest measured size not above it, a width the row of the smallest measured width not below it (the rule of section 8n).
//   n < 16        route 2 (n = 8: route 1 took 1.4 to 3.4 times as long)
//   16 <= n < 32  'A': route 2 (m = 1: 0.95, m = 4: 0.80)        'N': m <= 4 (1.05; m = 16: 0.87)
//   32 <= n < 64  'A': m <= 4 (1.28; m = 16: 0.65)               'N': every m (1.10 at m = 32)
//   n >= 64       every eligible cell (1.19 to 4.59)
bool groute1_measured_faster(int n, char mode, int m) {
  if (n < 16) return false;
  if (n < 32) return mode == 'N' && m <= 4;
  if (n < 64) return mode == 'A' ? m <= 4 : true;
  return true;
}

void gbrange_launch(const BatchArgs& g, int k0, int m, double accept, hipStream_t st, unsigned long long* first, int* redo) {
  with_n_class<EIGX_GBATCH_NMAX>(g.n, [&](auto nmax) {
    constexpr int NMAX = decltype(nmax)::value;
    constexpr int MW = NMAX <= 64 ? 16 : 0;
    hipLaunchKernelGGL((gbatch_range_kernel<NMAX, MW>), dim3((unsigned)g.batch), dim3(2 * NMAX), 0, st, g.n, g.batch, k0, m,
                       (const double*)g.a, g.lda, g.stride_a, g.b, g.ldb, g.stride_b, g.w, g.ldw, g.z, g.ldz, g.stride_z,
                       (int)(g.mode == 'A'), accept, g.info, first, redo);
  });
}

int gbrange_full_solve(const BatchArgs& c) {
  return eigx_gev_batch_dev(c.n, c.batch, c.a, c.lda, c.stride_a, c.b, c.ldb, c.stride_b, c.w, c.ldw, c.z, c.ldz, c.stride_z, c.mode,
                            c.info);
}

// (route 3 is gbatch_solve_window of gbatch.hip: eigx_gev_range_dev, an odd leading dimension staged as eigx_gev_batch does above
// its cutoff; the pool names are part of the description of the entry in include/eigenexa_amd_gbatch_range.h)
const WindowFamily gbrange_family{get_gbatch_nmax, gwindow_width, groute1_measured_faster, gbrange_launch, gbrange_full_solve,
                                  gbatch_solve_window, "gbrange.first", "gbrange.redo", "gbrange.rw", "gbrange.rz", "gbrange.rinfo",
                                  {"gbrange.ha", "gbrange.hb", "gbrange.hz", "gbrange.hw", "gbrange.hinfo"}};

}  // namespace
}  // namespace eigx

using namespace eigx;

extern "C" {

// EXTENSION: eigenpairs il .. iu of `batch` symmetric-definite pencils of one size (one GPU); see brange_frame_host /
// brange_frame_dev (batch_frame.hip)
int eigx_gev_batch_range(int n, int batch, int il, int iu, double* a, int lda, int64_t stride_a, double* b, int ldb, int64_t stride_b,
                         double* w, int ldw, double* z, int ldz, int64_t stride_z, char mode, int* info) {
  const BatchArgs g{n, batch, a, lda, stride_a, b, ldb, stride_b, w, ldw, z, ldz, stride_z, mode, info, 8, true};
  return eigx_guard(g_ctx, [&] { return brange_frame_host(g_ctx, g, il, iu, gbrange_family); });
}
int eigx_gev_batch_range_dev(int n, int batch, int il, int iu, double* a_dev, int lda, int64_t stride_a, double* b_dev, int ldb,
                             int64_t stride_b, double* w_dev, int ldw, double* z_dev, int ldz, int64_t stride_z, char mode,
                             int* info_dev) {
  const BatchArgs g{n, batch, a_dev, lda, stride_a, b_dev, ldb, stride_b, w_dev, ldw, z_dev, ldz, stride_z, mode, info_dev, 8, true};
  return eigx_guard(g_ctx, [&] { return brange_frame_dev(g_ctx, g, il, iu, gbrange_family); });
}

}  // extern "C"
