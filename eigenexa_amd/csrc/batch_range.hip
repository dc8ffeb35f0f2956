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
#include "eigx_context.h"
#include "batch_common.h"
#include "../../include/eigenexa_amd.h"
#include <algorithm>
#include <cfloat>
#include <vector>

#pragma clang fp contract(off)

namespace eigx {
namespace {

// Phase 2 of sym_tridiag_ql (batch_common.h) alone: the full symmetric matrix of order n in A(LD, NMAX) -> (d, e), e[i] coupling
// i - 1 and i, e[0] = 0; the reflector of step i stays in A(0 .. i-1, i), its h in hv[i] (0: no reflector).  The loop is that
// function's first loop word for word: calling this from there would move the code of the existing kernels (see the head of
// batch_common.h).  Every thread of the workgroup makes the call; the results are behind a barrier.
template <int NMAX>
__device__ __forceinline__ void sym_tridiag(int n, double* A, double* d, double* e, double* hv, double* u, double* q, double* pt,
                                            double (*red)[4]) {
  constexpr int NT = 2 * NMAX, LD = NMAX + 1;
  const int tid = threadIdx.x, r = tid % NMAX, hh = tid / NMAX;
  const bool row = hh == 0 && r < n;
  for (int i = n - 1; i >= 1; --i) {
    const int l = i - 1;
    double* rd = red[2 * (i & 1)];     // by parity: a step that leaves early has no closing barrier
    if (l == 0) {
      if (tid == 0) { e[1] = A[LD]; hv[1] = 0.0; }
      continue;
    }
    const double x = (hh == 0 && r <= l) ? A[r + i * LD] : 0.0;
    const double f = A[l + i * LD];    // (read before the barrier: thread l overwrites it below)
    double h = block_sum<NT>(x * x, rd);
    if (h == 0.0) {                    // nothing to annihilate (uniform)
      if (tid == 0) { e[i] = f; hv[i] = 0.0; }
      continue;
    }
    const double g = f >= 0.0 ? -sqrt(h) : sqrt(h);
    h -= f * g;
    if (hh == 0 && r <= l) {
      const double ur = r == l ? f - g : x;
      u[r] = ur;
      A[r + i * LD] = ur;
    }
    if (tid == 0) { e[i] = g; hv[i] = h; }
    __syncthreads();
    const int mid = (l + 2) / 2, k0 = hh ? mid : 0, k1 = hh ? l + 1 : mid;
    if (r <= l) {
      double acc = 0.0;
#pragma unroll 4
      for (int t = 0; t < mid; ++t) {
        const int c = k0 + t;
        const double uc = u[c];
        acc = fma(A[r + c * LD], c < k1 ? uc : 0.0, acc);
      }
      pt[hh * NMAX + r] = acc;
    }
    __syncthreads();
    double qr = 0.0, ur = 0.0;
    if (hh == 0 && r <= l) { ur = u[r]; qr = (pt[r] + pt[NMAX + r]) / h; }
    const double hk = block_sum<NT>(qr * ur, rd + 4) / (h + h);
    if (hh == 0 && r <= l) q[r] = qr - hk * ur;
    __syncthreads();
    if (r <= l) {
      ur = u[r];
      qr = q[r];
#pragma unroll 4
      for (int t = 0; t < mid; ++t) {
        const int c = k0 + t;
        const double ac = A[r + c * LD], qc = q[c], uc = u[c];
        A[r + c * LD] = c < k1 ? ac - (ur * qc + qr * uc) : ac;
      }
    }
    __syncthreads();
  }
  if (row) d[r] = A[r + r * LD];
  if (tid == 0) { e[0] = 0.0; hv[0] = 0.0; }
  __syncthreads();
}

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

// Route 2's second step: the window of the full solves of matrices kb .. kb + gridDim.x - 1 (rw(n, .), rz(n, n, .), rinfo: what
// eigx_s_batch_dev left in the workspace) -> the caller's w(1:m, k), z(1:n, 1:m, k), info[k] and the first-failure word.  A
// failed matrix: w(1:m, k) = NaN, z(:, :, k) untouched.
__global__ __launch_bounds__(256) void batch_range_gather(int n, int kb, int k0, int m, const double* __restrict__ rw,
                                                          const double* __restrict__ rz, const int* __restrict__ rinfo,
                                                          double* __restrict__ w, int ldw, double* __restrict__ z, int ldz,
                                                          int64_t stride_z, int want_vec, int* __restrict__ info,
                                                          unsigned long long* __restrict__ first) {
  const int kl = blockIdx.x, k = kb + kl, tid = threadIdx.x;
  const int code = rinfo[kl];
  double* wk = w + (size_t)k * ldw;
  if (code != 0) {
    for (int j = tid; j < m; j += 256) wk[j] = std::numeric_limits<double>::quiet_NaN();
    if (tid == 0) report_failure(first, info, k, code);
    return;
  }
  for (int j = tid; j < m; j += 256) wk[j] = rw[(size_t)kl * n + k0 + j];
  if (want_vec) {
    const double* src = rz + (size_t)kl * n * n + (size_t)k0 * n;
    double* zk = z + (size_t)k * stride_z;
    for (int idx = tid; idx < n * m; idx += 256) zk[idx % n + (size_t)(idx / n) * ldz] = src[idx];
  }
  if (tid == 0 && info) info[k] = 0;
}

// a call: the arguments of the entries (device or host arrays)
struct RangeBatchArgs {
  int n, batch, il, iu;
  double* a; int lda; int64_t stride_a;
  double* w; int ldw;
  double* z; int ldz; int64_t stride_z;
  char mode; int* info;
  int m() const { return iu - il + 1; }
};

int g_route_key = 0;       // key 26: 0 = automatic, 1 = route 1 wherever eligible, 2 = route 2 always
int g_accept_key = 50;     // key 27: the acceptance bound in percent

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

void brange_launch(const RangeBatchArgs& g, hipStream_t st, unsigned long long* first, int* redo) {
  with_n_class<EIGX_BATCH_NMAX>(g.n, [&](auto nmax) {
    constexpr int NMAX = decltype(nmax)::value;
    constexpr int MW = NMAX <= 96 ? 16 : 4;
    hipLaunchKernelGGL((batch_range_kernel<NMAX, MW>), dim3((unsigned)g.batch), dim3(2 * NMAX), 0, st, g.n, g.batch, g.il - 1, g.m(),
                       (const double*)g.a, g.lda, g.stride_a, g.w, g.ldw, g.z, g.ldz, g.stride_z, (int)(g.mode == 'A'),
                       g_accept_key / 100.0, g.info, first, redo);
  });
}

// Route 2 on matrices kb .. kb + cnt - 1: eigx_s_batch_dev into the workspace, chunk by chunk (at most 256 MiB of workspace), and
// the gather.  Returns EIGX_OK or a status that does not belong to one matrix.
int brange_full_and_slice(Context& ctx, const RangeBatchArgs& g, int kb, int cnt, unsigned long long* first) {
  const int n = g.n;
  const bool want_vec = g.mode == 'A';
  const size_t per = 8 * ((size_t)n + (want_vec ? (size_t)n * n : 0));
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)cnt, ((size_t)256 << 20) / per));
  double* rw = ctx.pool.get_t<double>("batch.rw", (size_t)n * chunk);
  double* rz = want_vec ? ctx.pool.get_t<double>("batch.rz", (size_t)n * n * chunk) : nullptr;
  int* rinfo = ctx.pool.get_t<int>("batch.rinfo", (size_t)chunk);
  for (int c0 = 0; c0 < cnt; c0 += chunk) {
    const int nc = std::min(chunk, cnt - c0), kc = kb + c0;
    const int rc = eigx_s_batch_dev(n, nc, g.a + (size_t)kc * g.stride_a, g.lda, g.stride_a, rw, n, rz, n, (int64_t)n * n, g.mode, rinfo);
    if (!batch_status_per_matrix(rc)) return rc;
    hipLaunchKernelGGL(batch_range_gather, dim3((unsigned)nc), dim3(256), 0, ctx.stream, n, kc, g.il - 1, g.m(), (const double*)rw,
                       (const double*)rz, (const int*)rinfo, g.w, g.ldw, g.z, g.ldz, g.stride_z, (int)want_vec, g.info, first);
    EIGX_HIP_CHECK(hipGetLastError());
    EIGX_HIP_CHECK(hipStreamSynchronize(ctx.stream));   // the next chunk overwrites the workspace
  }
  return EIGX_OK;
}

bool brange_args_ok(const RangeBatchArgs& g) {
  const int n = g.n, batch = g.batch;
  if (n < 1 || batch < 0 || g.il < 1 || g.iu > n || g.il > g.iu || g.lda < n || g.ldw < g.m() || (g.mode != 'A' && g.mode != 'N'))
    return false;
  if (batch > 1 && g.stride_a < (int64_t)g.lda * n) return false;
  if (g.mode == 'A' && (g.ldz < n || (batch > 1 && g.stride_z < (int64_t)g.ldz * g.m()))) return false;
  if (batch > 0 && (!g.a || !g.w || (g.mode == 'A' && !g.z))) return false;
  return true;
}

int brange_frame_dev(Context& ctx, RangeBatchArgs g) {
  int rc;
  if (!batch_entry_begin(ctx, g.mode, g.batch, [&] { return brange_args_ok(g); }, rc)) return rc;
  EIGX_HIP_CHECK(hipStreamSynchronize(nullptr));   // the caller's default-stream work on the arguments
  const double t0 = now_s();
  hipStream_t st = ctx.stream;
  const int n = g.n, batch = g.batch, m = g.m();
  int redone = 0;
  if (n > get_batch_nmax()) {
    // route 3: the index-range solver of one large matrix (eigx_s_range_dev with the interface's default block sizes), matrix by
    // matrix; unlike the uniform frame this one sets errinfo to -1 after a failed matrix (the table of DESIGN section 8h)
    set_batch_range_last(3, m, 0);
    rc = batch_loop_above_cutoff(batch, g.info, [&](int k) {
      return range_solve_dev(ctx, n, RangeWindow::index(g.il, g.iu), g.a + (size_t)k * g.stride_a, g.lda, g.w + (size_t)k * g.ldw,
                             g.mode == 'A' ? g.z + (size_t)k * g.stride_z : nullptr, g.ldz, 48, 128, g.mode, 1, false);
    });
    if (!batch_status_per_matrix(rc)) return rc;
    ctx.errinfo = rc == EIGX_OK ? 0 : -1;
  } else {
    const bool eligible = g.mode == 'N' || m <= window_width(n);
    const bool one = g_route_key == 2 ? false : eligible && (g_route_key == 1 || route1_measured_faster(n, g.mode, m));
    set_batch_range_last(one ? 1 : 2, m, 0);
    FirstFailure ff;                     // a word of its own: route 2's eigx_s_batch_dev arms batch.first while this one is live
    ff.arm(ctx, "brange.first", st);
    unsigned long long* first = ff.dev;
    if (one) {
      int* redo = ctx.pool.get_t<int>("brange.redo", (size_t)batch);
      brange_launch(g, st, first, redo);
      EIGX_HIP_CHECK(hipGetLastError());
      std::vector<int> marks((size_t)batch);
      EIGX_HIP_CHECK(hipMemcpyAsync(marks.data(), redo, (size_t)batch * sizeof(int), hipMemcpyDeviceToHost, st));
      EIGX_HIP_CHECK(hipStreamSynchronize(st));
      // the redo: route 2 on every run of consecutive marked matrices
      for (int k = 0; k < batch;) {
        if (!marks[k]) { ++k; continue; }
        int k1 = k;
        while (k1 < batch && marks[k1]) ++k1;
        const int rr = brange_full_and_slice(ctx, g, k, k1 - k, first);
        if (rr != EIGX_OK) return rr;
        set_batch_range_last(1, m, redone += k1 - k);
        k = k1;
      }
    } else {
      const int rr = brange_full_and_slice(ctx, g, 0, batch, first);
      if (rr != EIGX_OK) return rr;
    }
    ctx.errinfo = 0;
    ff.finish(ctx, st, rc);
  }
  batch_entry_end(ctx, t0);
  return rc;
}

// Host arrays: batch_stage_host (batch_frame.hip) with m columns of z and m entries of w per matrix, in pool buffers of this
// entry's own (brange.h*: the names are part of the description of the entry in include/eigenexa_amd_batch_range.h).
int brange_frame_host(Context& ctx, RangeBatchArgs g) {
  int rc;
  if (!batch_entry_begin(ctx, g.mode, g.batch, [&] { return brange_args_ok(g); }, rc)) return rc;
  const BatchArgs u{g.n, g.batch, g.a, g.lda, g.stride_a, nullptr, 0, 0, g.w, g.ldw, g.z, g.ldz, g.stride_z, g.mode, g.info, 8, false};
  static const BatchStageNames names{"brange.ha", nullptr, "brange.hz", "brange.hw", "brange.hinfo"};
  return batch_stage_host(ctx, u, g.m(), g.m(), names, [&](const BatchArgs& dv) {
    return brange_frame_dev(ctx, RangeBatchArgs{g.n, g.batch, g.il, g.iu, dv.a, dv.lda, dv.stride_a, dv.w, dv.ldw, dv.z, dv.ldz,
                                                dv.stride_z, g.mode, dv.info});
  });
}

}  // namespace

// what the last call of a windowed batched entry did (eigx_batch_range_info): written by this file's frame and by the Hermitian
// family's (hbatch_range.hip) through set_batch_range_last
static struct { int route = 0, m = 0, redone = 0; } g_last;
void set_batch_range_last(int route, int m, int redone) {
  g_last.route = route;
  g_last.m = m;
  g_last.redone = redone;
}
int get_batch_range_route() { return g_route_key; }
int get_batch_range_accept() { return g_accept_key; }

int set_batch_range_route(int v) {
  if (v < 0 || v > 2) return -1;
  const int old = g_route_key;
  g_route_key = v;
  return old;
}
int set_batch_range_accept(int v) {
  if (v < 0 || v > 101) return -1;
  const int old = g_accept_key;
  g_accept_key = v;
  return old;
}

}  // namespace eigx

using namespace eigx;

extern "C" {

// EXTENSION: eigenpairs il .. iu of `batch` symmetric matrices of one size (one GPU); see brange_frame_host / brange_frame_dev
int eigx_s_batch_range(int n, int batch, int il, int iu, double* a, int lda, int64_t stride_a, double* w, int ldw, double* z, int ldz,
                       int64_t stride_z, char mode, int* info) {
  const RangeBatchArgs g{n, batch, il, iu, a, lda, stride_a, w, ldw, z, ldz, stride_z, mode, info};
  return eigx_guard(g_ctx, [&] { return brange_frame_host(g_ctx, g); });
}
int eigx_s_batch_range_dev(int n, int batch, int il, int iu, double* a_dev, int lda, int64_t stride_a, double* w_dev, int ldw,
                           double* z_dev, int ldz, int64_t stride_z, char mode, int* info_dev) {
  const RangeBatchArgs g{n, batch, il, iu, a_dev, lda, stride_a, w_dev, ldw, z_dev, ldz, stride_z, mode, info_dev};
  return eigx_guard(g_ctx, [&] { return brange_frame_dev(g_ctx, g); });
}
int eigx_batch_range_info(int* route, int* m, int* redone) {
  if (route) *route = g_last.route;
  if (m) *m = g_last.m;
  if (redone) *redone = g_last.redone;
  return EIGX_OK;
}

}  // extern "C"
