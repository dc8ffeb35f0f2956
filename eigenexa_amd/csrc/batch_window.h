// batch_window.h -- the real tridiagonal window stage of a windowed one-workgroup-per-matrix kernel as device functions:
// eigenpairs k0 .. k0 + m - 1 of the real symmetric tridiagonal matrix (d, e) of order n held in LDS, without a QL sweep of the
// whole matrix (DESIGN sections 8n and 8o).  hbatch_range_kernel, gbatch_range_kernel and hgbatch_range_kernel, whose reductions
// end in a real (d, e), call them.  They are steps 3 to 6 of batch_range_kernel (batch_range.hip, real symmetric), which keeps those
// steps written out in its body and takes only sturm_count and start_entry from here: with the calls in their place that kernel
// compiled to other instructions (24 854 lines of ISA for 20 992, a spilled scalar register), and the existing entry is not to
// change (section 8o; an entry on section 8h's list of what stays written more than once).  One rule differs from that body: a
// pivot below ptiny counts as zero in the inverse iteration.
//   window_bounds        Gershgorin bounds, the pivot floor and the scale of the shifts
//   window_multisection  Sturm-count multi-section: a group of lanes per eigenvalue
//   window_inverse_iteration  one lane per vector on a tridiagonal LU with partial pivoting held in LDS
//   window_gram_schmidt  two passes over the window with the acceptance test (eigx_tune key 27)
//   window_rayleigh_ritz H = Y^T T Y on an m x m LDS tile through sym_tridiag_ql, Y <- Y S
// Every function is called by every thread of a workgroup of 2 NMAX threads, thread (r, hh) = (row, half) as in batch_kernel; MW is
// the widest window of mode 'A'; the window arrays F (4 NMAX MW) and Y (NMAX MW) hold entry (i, j) at [i MW + j] (lane-fastest).
// Every sum is taken in an order that depends on n and the window alone.
#pragma once
#include "batch_common.h"

#pragma clang fp contract(off)

namespace eigx {
namespace {

// the number of eigenvalues of the tridiagonal (d, e2 = e^2) below x; a pivot smaller than pivmin counts as -pivmin (DLAEBZ)
__device__ inline int sturm_count(int n, const double* d, const double* e2, double x, double pivmin) {
  double p = d[0] - x;
  if (fabs(p) < pivmin) p = -pivmin;
  int c = p < 0.0 ? 1 : 0;
  for (int i = 1; i < n; ++i) {
    p = d[i] - x - e2[i] / p;
    if (fabs(p) < pivmin) p = -pivmin;
    c += p < 0.0 ? 1 : 0;
  }
  return c;
}

// entry i of the start vector of window column j, in [-0.5, 0.5): a hash of (i, j) alone
__device__ inline double start_entry(int i, int j) {
  unsigned h = (unsigned)i * 2654435761u ^ ((unsigned)j * 40503u + 0x9e3779b9u);
  h ^= h >> 15; h *= 0x2c1b3c6du;
  h ^= h >> 12; h *= 0x297a2d39u;
  h ^= h >> 15;
  return (double)(h >> 8) * (1.0 / 16777216.0) - 0.5;
}

// what the stage knows of T before it starts: -gneg / gpos the Gershgorin bounds, tnorm = max(|gneg|, |gpos|) (0: the zero
// matrix), pivmin the floor of a Sturm pivot, epsT = eps tnorm
struct WindowBounds { double gneg, gpos, tnorm, pivmin, epsT; };

// Gershgorin bounds of (d, e), e[i] coupling i - 1 and i; e2 <- e^2, published by the last reduction's barrier
template <int NMAX>
__device__ __forceinline__ WindowBounds window_bounds(int n, const double* d, const double* e, double* e2, double (*red)[4]) {
  constexpr int NT = 2 * NMAX;
  const int tid = threadIdx.x, r = tid % NMAX, hh = tid / NMAX;
  const bool row = hh == 0 && r < n;
  double gneg = -DBL_MAX, gpos = -DBL_MAX, e2r = 0.0;
  if (row) {
    const double er = e[r], en = r + 1 < n ? e[r + 1] : 0.0, rad = fabs(er) + fabs(en);
    gneg = -(d[r] - rad);
    gpos = d[r] + rad;
    e2r = er * er;
    e2[r] = e2r;
  }
  gneg = block_max<NT>(gneg, red[0]);
  gpos = block_max<NT>(gpos, red[1]);
  e2r = block_max<NT>(e2r, red[2]);    // (its barrier publishes e2)
  WindowBounds b;
  b.gneg = gneg;
  b.gpos = gpos;
  b.tnorm = fmax(fabs(gneg), fabs(gpos));
  b.pivmin = DBL_MIN * fmax(1.0, e2r);
  b.epsT = DBL_EPSILON * b.tnorm;
  return b;
}

// Eigenvalue k0 + gj of (d, e2), gj = tid / G, by multi-section on Sturm counts with G = min(2 NMAX / m, 64) lanes per eigenvalue:
// the value is returned in every lane of group gj < m (what the lanes of the other groups get is not an eigenvalue).  cn: 2 NMAX
// ints, the counts of a round.  No closing barrier.
template <int NMAX>
__device__ __forceinline__ double window_multisection(int n, int k0, int m, const double* d, const double* e2, int* cn,
                                                      const WindowBounds& b) {
  constexpr int NT = 2 * NMAX;
  const int tid = threadIdx.x;
  const double pivmin = b.pivmin;
  const double wide = 2.1 * n * b.epsT + 2.1 * pivmin;
  const int G = NT / m < 64 ? NT / m : 64;          // lanes per eigenvalue (m <= n <= NMAX: at least 2)
  const int gj = tid / G, gs = tid % G;
  const int kk = k0 + gj;
  double lo = -b.gneg - wide, hi = b.gpos + wide;
  bool done = gj >= m;
  for (int round = 0; round < 1200; ++round) {   // (a round gains at least one bit: 1200 cover the denormals)
    const double step = (hi - lo) / (G + 1);
    if (!done) {
      const double x = fmin(fmax(lo + step * (gs + 1), lo), hi);
      cn[tid] = sturm_count(n, d, e2, x, pivmin);
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
  return lo + (hi - lo) * 0.5;
}

// Eigenvectors of T for the shifts lamv[0 .. m-1] (ascending, published): inverse iteration, lane j on T - lam_j I.  F: the four
// factor arrays; Y <- the normalised vectors; *bad = 1 (the caller has cleared it) where a lane met a vector without a norm.
// Behind a barrier.
template <int NMAX, int MW>
__device__ __forceinline__ void window_inverse_iteration(int n, int m, const double* d, const double* e, double* lamv, double* F,
                                                         double* Y, double epsT, int* bad) {
  const int tid = threadIdx.x;
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
    // LU with partial pivoting (DLAGTF): row i of U = (ua, ub, uc)[i], the multiplier of row i + 1 in ml[i].  A pivot below ptiny
    // counts as zero and becomes eps ||T|| (DLAGTS, job = -1): its reciprocal squared, which the norm of the solve sums, is not
    // finite.  Such pivots are met, not only in theory: a Hermitian matrix i K, K real antisymmetric of odd order, reduces to a
    // T with an exactly zero diagonal, the multi-section follows its eigenvalue 0 down to a denormal shift, and T - lam I has a
    // denormal last pivot.  (The inputs are scaled to max|a| >= 1e-90: nothing of T lives 48 orders below that.)
    const double ptiny = 6.7e-139;         // sqrt(DBL_MIN) / DBL_EPSILON
    double p = d[0] - lam, s = n > 1 ? e[1] : 0.0;
    for (int i = 0; i < n - 1; ++i) {
      const double sub = e[i + 1], dn = d[i + 1] - lam, en = i + 2 < n ? e[i + 2] : 0.0;
      double mult;
      if (fabs(p) >= fabs(sub)) {
        if (fabs(p) < ptiny) p = epsT;
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
    if (fabs(p) < ptiny) p = epsT;
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
        *bad = 1;
        break;
      }
      const double sc = 1.0 / sqrt(nrm);
      for (int i = 0; i < n; ++i) Y[i * MW + j] *= sc;
    }
  }
  __syncthreads();
}

// Two passes of Gram-Schmidt over the m columns of Y; in the second every vector has to keep `accept` of its norm.  pt: 2 NMAX
// partial sums, u: NMAX coefficients.  Returns true (uniform) where a vector was refused: Y is not orthonormal then.
template <int NMAX, int MW>
__device__ __forceinline__ bool window_gram_schmidt(int n, int m, double* Y, double* pt, double* u, double (*red)[4], double accept,
                                                    bool refused) {
  constexpr int NT = 2 * NMAX, CH = NT / MW;
  const int tid = threadIdx.x, r = tid % NMAX, hh = tid / NMAX;
  const bool row = hh == 0 && r < n;
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
  return refused;
}

// Rayleigh-Ritz: H = Y^T T Y, H = S W S^T (sym_tridiag_ql on the tile H(LD, m) at F + NMAX MW), lamv <- W ascending, F(0 .. n MW)
// <- Y S in that order.  d, e are destroyed with hv, u, q, pt (2 NMAX), ctl, msk: the scratch of sym_tridiag_ql.  Returns false
// (uniform) where the QL budget ran out; otherwise behind a barrier.
template <int NMAX, int MW>
__device__ __forceinline__ bool window_rayleigh_ritz(int n, int m, double* d, double* e, double* hv, double* u, double* q,
                                                     double* pt, double (*red)[4], int* ctl, unsigned long long* msk, double* F,
                                                     const double* Y, double* lamv, int* perm) {
  constexpr int NT = 2 * NMAX, LD = NMAX + 1;
  static_assert(NT % MW == 0 && (NMAX + 1) * MW <= 3 * NMAX * MW, "layout of the window storage");
  const int tid = threadIdx.x;
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
  if (sym_tridiag_ql<NMAX>(m, 1, Ht, d, e, hv, u, q, pt, red, ctl, msk) == ST_FAIL) return false;   // uniform
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
  return true;
}

}  // namespace
}  // namespace eigx
