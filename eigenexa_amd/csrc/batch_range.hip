// batch_range.hip -- eigx_s_batch_range (EXTENSION, not in the reference): eigenpairs il .. iu of many small symmetric matrices
// (n <= EIGX_BATCH_NMAX) in one launch, one workgroup per matrix, the matrix resident in LDS from load to store (DESIGN
// section 8n).  The window kernel (route 1):
//   load the upper triangle, mirror it, scan for NaN / Inf, scale (as batch_kernel, batch.hip)
//   -> Householder tridiagonalisation only (the first loop of sym_tridiag_ql: the reflectors stay in A's columns, Q is not formed)
//   -> Sturm-count multi-section on (d, e^2): a group of lanes per eigenvalue, no QL sweep
//   -> mode 'A': inverse iteration, one lane per vector, on a tridiagonal LU with partial pivoting held in LDS
//   -> two passes of Gram-Schmidt over the window with an acceptance test (every vector keeps key 27 percent of its norm in the
//      second pass) -> Rayleigh-Ritz on the m x m projection (sym_tridiag_ql on an LDS tile) -> the n - 1 reflectors applied to
//      the m columns -> unscale, store w(1:m), z(1:n, 1:m).
// No workgroup talks to another, no atomics on the data, every sum in an order that depends on n and the window alone.  A matrix
// the acceptance test refuses leaves a mark and is solved again by route 2: eigx_s_batch_dev into pooled workspace and a gather
// of the window (bit for bit the slice of that entry's result).  n above the cutoff of eigx_s_batch (eigx_tune key 21) goes
// through range_solve_dev matrix by matrix (route 3).  Which of routes 1 and 2 a call takes: eigx_tune key 26.
// This file holds the window kernel, the measured-route table and the family's WindowFamily record; the routes, the redo and the
// gather are the windowed frame's (batch_frame.hip), the reduction is sym_tridiag (batch_tridiag.h), sturm_count and start_entry
// are batch_window.h's.  The window stage itself stays written out in the kernel's body: see the head of batch_window.h.
#include "eigx_context.h"
#include "batch_common.h"
#include "batch_tridiag.h"
#include "batch_window.h"
#include "../../include/eigenexa_amd.h"
#include <cfloat>

#pragma clang fp contract(off)

namespace eigx {
namespace {

// One workgroup of 2 NMAX threads per matrix, thread (r, hh) = (row, half) as in batch_kernel.  MW: the widest window of mode 'A'.
// F: the four factor arrays of the inverse iteration, entry (i, j) at [i MW + j] (lane-fastest); later T Y, the projected
// matrix H(LD, m) and Y S.  Y: the vectors, the same layout.  k0 = il - 1, m = iu - il + 1; want_vec needs m <= MW.
// redo[k] = 1: the acceptance test refused matrix k and nothing of it was written.
template <int NMAX, int MW>
__global__ __launch_bounds__(2 * NMAX) void batch_range_kernel(int n, int batch, int k0, int m, const double* __restrict__ a, int lda,
                                                               int64_t stride_a, double* __restrict__ w, int ldw,
                                                               double* __restrict__ z, int ldz, int64_t stride_z, int want_vec,
                                                               double accept, int* __restrict__ info,
                                                               unsigned long long* __restrict__ first, int* __restrict__ redo) {
  constexpr int NT = 2 * NMAX, LD = NMAX + 1, CH = NT / MW;
  static_assert(NT % MW == 0 && (NMAX + 1) * MW <= 3 * NMAX * MW, "layout of the window storage");
  __shared__ double A[LD * NMAX];
  __shared__ double d[NMAX], e[NMAX], hv[NMAX], u[NMAX], q[NMAX], hs[NMAX];
  __shared__ double pt[2 * NMAX];        // partial sums; the counts of a multi-section round; (c_i, s_i) of a QL iteration
  __shared__ double red[4][4];
  __shared__ double F[4 * NMAX * MW];
  __shared__ double Y[NMAX * MW];
  __shared__ double lamv[MW];
  __shared__ int perm[MW];
  __shared__ int ctl[4];
  __shared__ int bad;                    // a lane of the inverse iteration met a vector without a norm
  __shared__ unsigned long long msk[2];
  const int tid = threadIdx.x, r = tid % NMAX, hh = tid / NMAX;
  const bool row = hh == 0 && r < n;

  for (int k = blockIdx.x; k < batch; k += gridDim.x) {
    // ---- 1. load the upper triangle, mirror, scan, scale (batch_kernel) ------------------------------------------------------
    const double* ak = a + (size_t)k * stride_a;
    double mx = 0.0, nf = 0.0;
    for (int j = hh; j < n; j += 2) {
      if (r <= j) {
        const double x = ak[r + (size_t)j * lda];
        if (!(fabs(x) <= DBL_MAX)) nf = 1.0;
        else mx = fmax(mx, fabs(x));
        A[r + j * LD] = x;
        A[j + r * LD] = x;
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
        for (int j = hh; j < n; j += 2) A[r + j * LD] *= sigma;
    }
    if (tid == 0) bad = 0;
    __syncthreads();

    // ---- 2. tridiagonalisation only ---------------------------------------------------------------------------------------------
    sym_tridiag<NMAX>(n, A, d, e, hv, u, q, pt, red);

    // ---- 3. eigenvalues k0 .. k0 + m - 1 by multi-section on Sturm counts ------------------------------------------------------
    // Gershgorin bounds, widened; q <- e^2
    double gneg = -DBL_MAX, gpos = -DBL_MAX, e2r = 0.0;
    if (row) {
      const double er = e[r], en = r + 1 < n ? e[r + 1] : 0.0, rad = fabs(er) + fabs(en);
      gneg = -(d[r] - rad);
      gpos = d[r] + rad;
      e2r = er * er;
      q[r] = e2r;
    }
    gneg = block_max<NT>(gneg, red[0]);
    gpos = block_max<NT>(gpos, red[1]);
    e2r = block_max<NT>(e2r, red[2]);    // (its barrier publishes q)
    const double tnorm = fmax(fabs(gneg), fabs(gpos));
    const double pivmin = DBL_MIN * fmax(1.0, e2r);
    const double epsT = DBL_EPSILON * tnorm;
    if (tnorm == 0.0) {                  // the zero matrix (uniform): w = 0 exactly, unit vectors
      if (want_vec && !(1.0 >= accept)) {   // (their norm is 1: a bound above it refuses them like any others)
        if (tid == 0) redo[k] = 1;
        __syncthreads();
        continue;
      }
      if (tid < m) w[(size_t)k * ldw + tid] = 0.0;
      if (want_vec && r < n) {
        double* zk = z + (size_t)k * stride_z;
        for (int c = hh; c < m; c += 2) zk[r + (size_t)c * ldz] = r == k0 + c ? 1.0 : 0.0;
      }
      if (tid == 0) {
        if (info) info[k] = 0;
        redo[k] = 0;
      }
      __syncthreads();
      continue;
    }
    {
      const double wide = 2.1 * n * epsT + 2.1 * pivmin;
      const int G = NT / m < 64 ? NT / m : 64;          // lanes per eigenvalue (m <= n <= NMAX: at least 2)
      const int gj = tid / G, gs = tid % G;
      const int kk = k0 + gj;
      int* cn = (int*)pt;
      double lo = -gneg - wide, hi = gpos + wide;
      bool done = gj >= m;
      for (int round = 0; round < 1200; ++round) {   // (a round gains at least one bit: 1200 cover the denormals)
        const double step = (hi - lo) / (G + 1);
        if (!done) {
          const double x = fmin(fmax(lo + step * (gs + 1), lo), hi);
          cn[tid] = sturm_count(n, d, q, x, pivmin);
        }
        __syncthreads();
        if (!done) {
          int t = 0;                     // the points with at most kk eigenvalues below them: the first t of the group
          for (int s = 0; s < G; ++s) t += cn[gj * G + s] <= kk ? 1 : 0;
          const double nlo = t > 0 ? fmin(fmax(lo + step * t, lo), hi) : lo;
          const double nhi = t < G ? fmin(fmax(lo + step * (t + 1), lo), hi) : hi;
          done = nlo == lo && nhi == hi; // the points no longer separate the ends
          lo = nlo;
          hi = nhi;
        }
        if (!__syncthreads_or(done ? 0 : 1)) break;
      }
      const double lam = lo + (hi - lo) * 0.5;
      if (gj < m && gs == 0) {
        if (want_vec) lamv[gj] = lam;
        else w[(size_t)k * ldw + gj] = lam * unscale;
      }
    }
    if (!want_vec) {                     // uniform
      if (tid == 0) {
        if (info) info[k] = 0;
        redo[k] = 0;
      }
      __syncthreads();
      continue;
    }
    __syncthreads();

    // ---- 4. eigenvectors of T: inverse iteration, lane j on T - lam_j I ---------------------------------------------------------
    // shifts closer than 10 eps |lam_j| are moved apart (DSTEIN's rule).  The distance is relative to the shift, not to ||T||:
    // 10 eps ||T|| per column added up to 150 eps ||T|| across a window of 16 near-zero eigenvalues of a graded matrix, past
    // eigenvalues outside the window, and the window came back with the pairs of other indices
    if (tid == 0)
      for (int j = 1; j < m; ++j) {
        const double sep = 10.0 * DBL_EPSILON * fabs(lamv[j]);
        if (lamv[j] - lamv[j - 1] < sep) lamv[j] = lamv[j - 1] + sep;
      }
    __syncthreads();
    double* ua = F;
    double* ub = F + NMAX * MW;
    double* uc = F + 2 * NMAX * MW;
    double* ml = F + 3 * NMAX * MW;
    if (tid < m) {
      const int j = tid;
      const double lam = lamv[j];
      unsigned long long sw0 = 0, sw1 = 0;   // bit i: rows i and i + 1 were interchanged
      // LU with partial pivoting (DLAGTF): row i of U = (ua, ub, uc)[i], the multiplier of row i + 1 in ml[i]
      double p = d[0] - lam, s = n > 1 ? e[1] : 0.0;
      for (int i = 0; i < n - 1; ++i) {
        const double sub = e[i + 1], dn = d[i + 1] - lam, en = i + 2 < n ? e[i + 2] : 0.0;
        double mult;
        if (fabs(p) >= fabs(sub)) {
          if (p == 0.0) p = epsT;
          mult = sub / p;
          ua[i * MW + j] = p; ub[i * MW + j] = s; uc[i * MW + j] = 0.0;
          p = dn - mult * s;
          s = en;
        } else {
          mult = p / sub;
          ua[i * MW + j] = sub; ub[i * MW + j] = dn; uc[i * MW + j] = en;
          p = s - mult * dn;
          s = -(mult * en);
          if (i < 64) sw0 |= 1ull << i;
          else sw1 |= 1ull << (i - 64);
        }
        ml[i * MW + j] = mult;
      }
      if (p == 0.0) p = epsT;
      ua[(n - 1) * MW + j] = p; ub[(n - 1) * MW + j] = 0.0; uc[(n - 1) * MW + j] = 0.0;
      for (int i = 0; i < n; ++i) Y[i * MW + j] = start_entry(i, j);
      // the start is back-substituted, then two whole solves; each result normalised
      for (int sweep = 0; sweep < 3; ++sweep) {
        if (sweep > 0) {
          double xc = Y[j];
          for (int i = 0; i < n - 1; ++i) {
            double xn = Y[(i + 1) * MW + j];
            const bool swp = i < 64 ? (sw0 >> i) & 1 : (sw1 >> (i - 64)) & 1;
            if (swp) { const double t = xc; xc = xn; xn = t; }
            Y[i * MW + j] = xc;
            xc = xn - ml[i * MW + j] * xc;
          }
          Y[(n - 1) * MW + j] = xc;
        }
        double x1 = 0.0, x2 = 0.0, nrm = 0.0;
        for (int i = n - 1; i >= 0; --i) {
          const double x = (Y[i * MW + j] - ub[i * MW + j] * x1 - uc[i * MW + j] * x2) / ua[i * MW + j];
          Y[i * MW + j] = x;
          nrm = fma(x, x, nrm);
          x2 = x1;
          x1 = x;
        }
        if (!(nrm > 0.0 && nrm <= DBL_MAX)) {
          bad = 1;
          break;
        }
        const double sc = 1.0 / sqrt(nrm);
        for (int i = 0; i < n; ++i) Y[i * MW + j] *= sc;
      }
    }
    __syncthreads();
    bool refused = bad != 0;             // uniform

    // ---- 5. two passes of Gram-Schmidt over the window; the acceptance test in the second ------------------------------------------
    const int wc = tid % MW, wch = tid / MW;   // thread (column, chunk of rows) of the window-wide sums
    for (int pass = 0; pass < 2 && !refused; ++pass) {
      for (int j = 0; j < m; ++j) {
        double acc = 0.0;
        if (wc < j)
          for (int i = wch; i < n; i += CH) acc = fma(Y[i * MW + wc], Y[i * MW + j], acc);
        pt[tid] = acc;
        __syncthreads();
        if (tid < j) {
          double s = pt[tid];
          for (int c = 1; c < CH; ++c) s += pt[c * MW + tid];
          u[tid] = s;
        }
        __syncthreads();
        double v = 0.0;
        if (row) {
          v = Y[r * MW + j];
          for (int p = 0; p < j; ++p) v = fma(-u[p], Y[r * MW + p], v);
        }
        const double nr = sqrt(block_sum<NT>(v * v, red[j & 1]));
        if (pass == 0 ? !(nr > 0.0 && nr <= DBL_MAX) : !(nr >= accept)) refused = true;   // (a NaN refuses)
        if (row) Y[r * MW + j] = refused ? v : v / nr;
        __syncthreads();
      }
    }
    if (refused) {                       // uniform: route 2 solves this matrix again
      if (tid == 0) redo[k] = 1;
      __syncthreads();
      continue;
    }

    // ---- 6. Rayleigh-Ritz: H = Y^T T Y, H = S W S^T, Y <- Y S ---------------------------------------------------------------------
    double* V = F;                       // T Y, later Y S
    double* Ht = F + NMAX * MW;          // H(LD, m)
    for (int idx = tid; idx < n * MW; idx += NT) {
      const int i = idx / MW, c = idx % MW;
      if (c < m) {
        double v = d[i] * Y[idx];
        if (i > 0) v = fma(e[i], Y[idx - MW], v);
        if (i + 1 < n) v = fma(e[i + 1], Y[idx + MW], v);
        V[idx] = v;
      }
    }
    if (row) hs[r] = hv[r];
    __syncthreads();
    for (int idx = tid; idx < m * m; idx += NT) {
      const int p = idx % m, c = idx / m;
      if (p <= c) {
        double s = 0.0;
        for (int i = 0; i < n; ++i) s = fma(Y[i * MW + p], V[i * MW + c], s);
        Ht[p + c * LD] = s;
        Ht[c + p * LD] = s;
      }
    }
    __syncthreads();
    if (sym_tridiag_ql<NMAX>(m, 1, Ht, d, e, hv, u, q, pt, red, ctl, msk) == ST_FAIL) {   // uniform
      if (tid == 0) redo[k] = 1;
      __syncthreads();
      continue;
    }
    if (tid < m) {
      const int rank = ascending_rank(m, d, tid);
      perm[rank] = tid;
      lamv[rank] = d[tid];
    }
    __syncthreads();
    for (int idx = tid; idx < n * MW; idx += NT) {
      const int i = idx / MW, c = idx % MW;
      if (c < m) {
        const double* sc = Ht + perm[c] * LD;
        double s = 0.0;
        for (int p = 0; p < m; ++p) s = fma(Y[i * MW + p], sc[p], s);
        V[idx] = s;
      }
    }
    __syncthreads();

    // ---- 7. back-transformation: Z = H_{n-1} ... H_1 (Y S), the order of sym_tridiag_ql's second loop ------------------------------
    for (int i = 1; i < n; ++i) {
      const double h = hs[i];
      if (h == 0.0) continue;            // uniform
      const int l = i - 1;
      double acc = 0.0;
      if (wc < m)
        for (int t = wch; t <= l; t += CH) acc = fma(A[t + i * LD], V[t * MW + wc], acc);
      pt[tid] = acc;
      __syncthreads();
      if (tid < m) {
        double s = pt[tid];
        for (int c = 1; c < CH; ++c) s += pt[c * MW + tid];
        u[tid] = s / h;
      }
      __syncthreads();
      if (r <= l) {
        const double ur = A[r + i * LD];
        for (int c = hh; c < m; c += 2) V[r * MW + c] = fma(-u[c], ur, V[r * MW + c]);
      }
      __syncthreads();
    }
    if (tid < m) w[(size_t)k * ldw + tid] = lamv[tid] * unscale;
    if (r < n) {
      double* zk = z + (size_t)k * stride_z;
      for (int c = hh; c < m; c += 2) zk[r + (size_t)c * ldz] = V[r * MW + c];
    }
    if (tid == 0) {
      if (info) info[k] = 0;
      redo[k] = 0;
    }
    __syncthreads();
  }
}

// the widest window the class of n serves in mode 'A'
int window_width(int n) { return n <= 96 ? 16 : 4; }

// The automatic rule of key 26 = 0, read off the table of DESIGN section 8n (profiles/batch_range_time.log): route 1 where it
// measured not slower than route 2.  Measured at n = 8, 16, 32, 64, 96, 128 and m = 1, 4, MW (mode 'N' also m = n); a size takes the
// row of the largest measured size not above it, a width the row of the smallest measured width not below it (route 1's time
// grows with m, route 2's does not).
//   n < 16        route 2 (n = 8: route 1 took 1.4 to 3.9 times as long)
//   16 <= n < 32  'A': m = 1 (1.07 times faster; m = 4: 0.87)   'N': m <= 4 (1.28; m = 16: 0.99)
//   32 <= n < 64  'A': m <= 4 (1.67; m = 16: 0.73)              'N': every m (1.42 at m = 32)
//   n >= 64       every eligible cell (1.64 to 9.3)
bool route1_measured_faster(int n, char mode, int m) {
  if (n < 16) return false;
  if (n < 32) return mode == 'A' ? m == 1 : m <= 4;
  if (n < 64) return mode == 'A' ? m <= 4 : true;
  return true;
}

void brange_launch(const BatchArgs& g, int k0, int m, double accept, hipStream_t st, unsigned long long* first, int* redo) {
  with_n_class<EIGX_BATCH_NMAX>(g.n, [&](auto nmax) {
    constexpr int NMAX = decltype(nmax)::value;
    constexpr int MW = NMAX <= 96 ? 16 : 4;
    hipLaunchKernelGGL((batch_range_kernel<NMAX, MW>), dim3((unsigned)g.batch), dim3(2 * NMAX), 0, st, g.n, g.batch, k0, m,
                       (const double*)g.a, g.lda, g.stride_a, g.w, g.ldw, g.z, g.ldz, g.stride_z, (int)(g.mode == 'A'), accept, g.info,
                       first, redo);
  });
}

int brange_full_solve(const BatchArgs& c) {
  return eigx_s_batch_dev(c.n, c.batch, c.a, c.lda, c.stride_a, c.w, c.ldw, c.z, c.ldz, c.stride_z, c.mode, c.info);
}

// route 3: eigx_s_range_dev with the interface's default block sizes on matrix k
int brange_solve_window(Context& ctx, const BatchArgs& g, int k, int il, int iu) {
  return range_solve_dev(ctx, g.n, RangeWindow::index(il, iu), g.block(g.a, g.stride_a, k), g.lda, g.w + (size_t)k * g.ldw,
                         g.mode == 'A' ? g.block(g.z, g.stride_z, k) : nullptr, g.ldz, 48, 128, g.mode, 1, false);
}

// (the pool names are part of the description of the entry in include/eigenexa_amd_batch_range.h)
const WindowFamily brange_family{get_batch_nmax, window_width, route1_measured_faster, brange_launch, brange_full_solve,
                                 brange_solve_window, "brange.first", "brange.redo", "batch.rw", "batch.rz", "batch.rinfo",
                                 {"brange.ha", nullptr, "brange.hz", "brange.hw", "brange.hinfo"}};

}  // namespace
}  // namespace eigx

using namespace eigx;

extern "C" {

// EXTENSION: eigenpairs il .. iu of `batch` symmetric matrices of one size (one GPU); see brange_frame_host / brange_frame_dev
// (batch_frame.hip)
int eigx_s_batch_range(int n, int batch, int il, int iu, double* a, int lda, int64_t stride_a, double* w, int ldw, double* z, int ldz,
                       int64_t stride_z, char mode, int* info) {
  const BatchArgs g{n, batch, a, lda, stride_a, nullptr, 0, 0, w, ldw, z, ldz, stride_z, mode, info, 8, false};
  return eigx_guard(g_ctx, [&] { return brange_frame_host(g_ctx, g, il, iu, brange_family); });
}
int eigx_s_batch_range_dev(int n, int batch, int il, int iu, double* a_dev, int lda, int64_t stride_a, double* w_dev, int ldw,
                           double* z_dev, int ldz, int64_t stride_z, char mode, int* info_dev) {
  const BatchArgs g{n, batch, a_dev, lda, stride_a, nullptr, 0, 0, w_dev, ldw, z_dev, ldz, stride_z, mode, info_dev, 8, false};
  return eigx_guard(g_ctx, [&] { return brange_frame_dev(g_ctx, g, il, iu, brange_family); });
}

}  // extern "C"
