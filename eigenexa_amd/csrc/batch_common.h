// batch_common.h -- what the one-workgroup-per-matrix kernels share (batch.hip: real symmetric, hbatch.hip: complex
// Hermitian, gbatch.hip: real symmetric-definite pencils, hgbatch.hip: complex Hermitian-definite pencils): the workgroup
// reductions, the scaling rule, the failure word of a launch and the exit of a failed matrix, thread 0's QL sweep on a real (d, e)
// held in LDS, the rank of the sort, for the two real kernels the whole reduction + QL of a matrix held in LDS (sym_tridiag_ql)
// and for the two complex ones the same on split planes (herm_tridiag_ql).  The QL round loop is written in both: as a function
// of its own, called from both, it changed the register allocation and block placement of the real kernels and cost
// eigx_gev_batch 1.5 to 3 % at n <= 32 (profiles/batch_frame_bits.log).  For the same reason batch_kernel and hbatch_kernel keep
// the scaling rule written out (scale_exponent here serves gbatch_kernel and hgbatch_kernel) and hbatch_kernel its rank count:
// one instruction more in the prologue moves all the code behind it; with both helpers in use batch_kernel<64> measured 5 % and
// hbatch_kernel<96> 1 % slower (the intermediate form in profiles/batch_frame_bits.log).  The move of hbatch_kernel's phases
// into herm_tridiag_ql changed its register allocation but neither a bit of its results nor, beyond the spread of the repeats,
// its time (profiles/hgbatch_hbatch_bits.log).
#pragma once
#include <cfloat>
#include <cstdint>
#include <limits>
#include <hip/hip_runtime.h>

// a*b + c is written out as fma() where it is wanted (batch.hip, hbatch.hip: the rank-2 update has to round alike on both sides)
#pragma clang fp contract(off)

namespace eigx {
namespace {

constexpr int QL_MAXIT = 30;          // QL iterations per eigenvalue, counted over the matrix as LAPACK's dsteqr counts them: 30 n
                                      // in all (the first eigenvalue of a graded matrix of n = 100 takes more than 30, the rest few)
constexpr int ST_RUN = 0, ST_DONE = 1, ST_FAIL = 2;

// Sum / maximum of v over the workgroup (NT threads), the same value in every thread.  Butterfly inside each wave, then the
// wave partials in wave order: the order of the additions is a function of the thread index only.  One barrier; the caller
// keeps `part` (NT / 64 entries) alive until a later barrier.
template <int NT>
__device__ inline double block_sum(double v, double* part) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = part[0];
  for (int q = 1; q < NT / 64; ++q) s += part[q];
  return s;
}
template <int NT>
__device__ inline double block_max(double v, double* part) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = part[0];
  for (int q = 1; q < NT / 64; ++q) s = fmax(s, part[q]);
  return s;
}

// sqrt(f^2 + g^2): plain where neither square can overflow nor the larger one underflow
__device__ inline double hypot2(double f, double g) {
  const double m = fmax(fabs(f), fabs(g));
  if (m > 1e-140 && m < 1e140) return sqrt(fma(f, f, g * g));
  return hypot(f, g);
}

// the first set bit at or above position l of the 128 bits msk[0], msk[1] (the caller keeps one set)
__device__ inline int first_set_from(const unsigned long long* msk, int l) {
  if (l < 64) {
    const unsigned long long v = msk[0] >> l;
    if (v) return l + __ffsll(v) - 1;
    l = 64;
  }
  return l + __ffsll(msk[1] >> (l - 64)) - 1;
}

// first failed matrix of the launch: the smallest (index << 8 | -code) wins
__device__ inline void report_failure(unsigned long long* first, int* info, int k, int code) {
  if (info) info[k] = code;
  atomicMin(first, ((unsigned long long)k << 8) | (unsigned long long)(-code));
}
// Matrix k of the launch failed with `code` (uniform over the workgroup): w(1:n, k) = NaN by the row threads (row: this is the
// thread of row r), the failure word, a barrier.  The caller goes on with its next matrix.
__device__ inline void fail_matrix(int k, int code, bool row, int r, double* w, int ldw, int* info, unsigned long long* first) {
  if (row) w[(size_t)k * ldw + r] = std::numeric_limits<double>::quiet_NaN();
  if (threadIdx.x == 0) report_failure(first, info, k, code);
  __syncthreads();
}
// The same for a workgroup that serves one block and ends with it (gvbatch.hip; hgbatch.hip, whose kernel serves the uniform and
// the ragged entry): the block's eigenvalues are at wk, k is its caller index; no barrier.
__device__ inline void fail_block(int k, int code, bool row, int r, double* wk, int* info, unsigned long long* first) {
  if (row) wk[r] = std::numeric_limits<double>::quiet_NaN();
  if (threadIdx.x == 0) report_failure(first, info, k, code);
}

// the exponent ex of the scaling 2^-ex of a matrix whose largest entry is mx: 0 inside [1e-90, 1e90] (and for the zero
// matrix), else that of the power of two nearest to mx (eigen_scaling, solver.hip); even: rounded up to an even number
__device__ inline int scale_exponent(double mx, bool even) {
  if (!(mx > 0.0 && (mx < 1e-90 || mx > 1e90))) return 0;
  int ex = 0;
  (void)frexp(mx, &ex);
  ex = ex < -1000 ? -1000 : ex;        // (a denormal maximum: 2^-ex has to stay finite)
  return even ? ex + (ex & 1) : ex;
}

// One lane's part of a QL round on the real tridiagonal (d, e) of order n in LDS (tql2 / dsteqr): step ql_l over the converged
// eigenvalues, find the end m of the unreduced block in msk (bit m = e[m] is negligible) and make one sweep with Wilkinson
// shift: the rotations (c_i, s_i), i = m-1 .. l, go into pt, their range into ctl[0] (m) and ctl[1] (the lowest), the state
// into ctl[2].  ql_it counts the sweeps of the matrix.
__device__ inline void ql_sweep(int n, double* d, double* e, double* pt, int* ctl, const unsigned long long* msk, int& ql_l,
                                int& ql_it) {
        int st = ST_RUN, l = ql_l, m = 0;
        for (; l < n; ++l) {
          m = first_set_from(msk, l);
          if (m != l) break;
        }
        ql_l = l;
        if (l >= n) st = ST_DONE;
        else if (ql_it == QL_MAXIT * n) st = ST_FAIL;
        else {
          ++ql_it;
          const double dl = d[l], el = e[l];
          double g = (d[l + 1] - dl) / (2.0 * el);
          double rr = hypot2(g, 1.0);
          g = d[m] - dl + el / (g + copysign(rr, g));
          double s = 1.0, c = 1.0, p = 0.0;
          // d[i+1] is carried in a register, e[i-1] and d[i-1] are read one rotation ahead: no LDS round trip on the chain
          double dn = d[m], ei = e[m - 1], di = d[m - 1];
          int i = m - 1;
          for (; i >= l; --i) {
            const int ip = i > l ? i - 1 : l;       // (the last rotation reads ahead what it has already)
            const double e2 = e[ip], d2 = d[ip];
            const double f = s * ei, b = c * ei;
            rr = hypot2(f, g);
            e[i + 1] = rr;
            if (rr == 0.0) {             // recover from underflow: the block splits here
              d[i + 1] = dn - p;
              e[m] = 0.0;
              break;
            }
            const double ri = 1.0 / rr;
            s = f * ri;
            c = g * ri;
            g = dn - p;
            rr = (di - g) * s + 2.0 * c * b;
            p = s * rr;
            d[i + 1] = g + p;
            g = c * rr - b;
            pt[2 * i] = c;
            pt[2 * i + 1] = s;
            dn = di; ei = e2; di = d2;
          }
          if (i < l) {
            d[l] = dn - p;
            e[l] = g;
            e[m] = 0.0;
          }
          ctl[0] = m;
          ctl[1] = i + 1;                // rotations m-1 .. i+1 were made
        }
        ctl[2] = st;
}

// Phases 2 and 3 of a one-workgroup-per-matrix real symmetric solve (batch.hip: eigx_s_batch, gbatch.hip: eigx_gev_batch), 2 NMAX
// threads, thread (r, hh) = (row, half): the full symmetric matrix of order n in A(LD, NMAX), LD = NMAX + 1 -> Householder
// tridiagonalisation (tred2), Q accumulated in place in A (want_vec) -> implicit QL with Wilkinson shift on (d, e) with the
// rotations applied to A's rows.  Every array is the caller's LDS: d, e, hv, u, q of NMAX entries, pt of 2 NMAX, red[4][4], ctl[4],
// msk[2].  The caller has published A with a barrier; every thread of the workgroup makes the call and gets the same state back:
// ST_DONE (d holds the eigenvalues in the order of A's columns) or ST_FAIL (the QL budget is used up); both behind a barrier.
template <int NMAX>
__device__ __forceinline__ int sym_tridiag_ql(int n, int want_vec, double* A, double* d, double* e, double* hv, double* u, double* q,
                                              double* pt, double (*red)[4], int* ctl, unsigned long long* msk) {
  constexpr int NT = 2 * NMAX, LD = NMAX + 1;
  const int tid = threadIdx.x, r = tid % NMAX, hh = tid / NMAX;
  const bool row = hh == 0 && r < n;     // the thread that owns row r where one thread per row is wanted
  // ---- 2. tridiagonalisation, i = n-1 .. 1: H_i = I - u u^T / h annihilates A(0 .. i-2, i) (tred2) ------------------------
  // u stays in A(0 .. i-1, i), h in hv[i]; the active matrix is the full symmetric block 0 .. i-1
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
    // p = A u, each half over its share of the columns.  Both halves make mid steps (a uniform trip count lets the loop be
    // unrolled and its LDS reads be batched); the step that half 1 may have too many reads column l+1 and adds nothing
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
    // A <- A - u q^T - q u^T on the whole block (both triangles, rounded alike)
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

  // ---- Q = H_{n-1} ... H_1 accumulated in place, i = 0 .. n-1 (tred2's second loop) -----------------------------------
  if (want_vec) {
    if (r < n)
      for (int c = hh; c < r; c += 2) A[r + c * LD] = 0.0;   // the strict lower triangle: rows of the identity to be
    __syncthreads();
    for (int i = 0; i < n; ++i) {
      const int l = i - 1;
      if (hh == 0 && r <= l) { u[r] = A[r + i * LD]; A[r + i * LD] = 0.0; }
      if (hh == 0 && r == i) A[i + i * LD] = 1.0;
      const double h = hv[i];
      if (l < 0 || h == 0.0) continue;                       // uniform; the next step's first barrier publishes column i
      __syncthreads();
      const int mid = (l + 2) / 2, k0 = hh ? mid : 0, k1 = hh ? l + 1 : mid;
      if (r <= l) {                                          // g = Q^T u: lane = column
        double acc = 0.0;
#pragma unroll 4
        for (int t = 0; t < mid; ++t) {
          const int c = k0 + t;
          const double uc = u[c];
          acc = fma(c < k1 ? uc : 0.0, A[c + r * LD], acc);
        }
        pt[hh * NMAX + r] = acc;
      }
      __syncthreads();
      if (hh == 0 && r <= l) q[r] = (pt[r] + pt[NMAX + r]) / h;
      __syncthreads();
      if (r <= l) {                                          // Q <- Q - u g^T / h: lane = row
        const double ur = u[r];
#pragma unroll 4
        for (int t = 0; t < mid; ++t) {
          const int c = k0 + t;
          const double ac = A[r + c * LD], qc = q[c];
          A[r + c * LD] = c < k1 ? fma(-qc, ur, ac) : ac;
        }
      }
      __syncthreads();
    }
  }
  __syncthreads();

  // ---- 3. implicit QL with Wilkinson shift on (d, e) (tql2) -------------------------------------------------------------
  // A round: the row threads apply the rotations of the last sweep to Q and test every e[m] against its neighbours (one
  // ballot per wave: bit m of msk = "e[m] is negligible"; bit n-1 is always set) -> barrier -> thread 0 steps l over the
  // converged eigenvalues, finds the end m of the unreduced block in msk and makes one sweep: the rotations (c_i, s_i),
  // i = m-1 .. l, go into pt -> barrier.  Two barriers per QL iteration, reached by every thread.
  int ql_l = 0, ql_it = 0;
  if (tid == 0) {
    for (int i = 1; i < n; ++i) e[i - 1] = e[i];
    e[n - 1] = 0.0;
    ctl[0] = 0;                        // no rotations yet
    ctl[1] = 1;
    msk[1] = 0;
  }
  __syncthreads();
  for (;;) {
    {
      const int m = ctl[0], lo = ctl[1];
      if (want_vec && row && lo < m) {
        double hc = A[r + m * LD];
#pragma unroll 4
        for (int i = m - 1; i >= lo; --i) {
          const double zi = A[r + i * LD], c = pt[2 * i], s = pt[2 * i + 1];
          A[r + (i + 1) * LD] = fma(s, zi, c * hc);
          hc = fma(c, zi, -(s * hc));
        }
        A[r + lo * LD] = hc;
      }
      bool small = false;
      if (row) small = r == n - 1 || fabs(e[r]) <= (0.5 * DBL_EPSILON) * (fabs(d[r]) + fabs(d[r + 1]));
      const unsigned long long bits = __ballot(small);
      if ((tid & 63) == 0 && tid < 128) msk[tid >> 6] = bits;   // (rows live in threads 0 .. n-1; the lanes of half 1 vote 0)
    }
    __syncthreads();
    if (tid == 0) ql_sweep(n, d, e, pt, ctl, msk, ql_l, ql_it);
    __syncthreads();
    if (ctl[2] != ST_RUN) break;
  }
  return ctl[2];
}

// Phases 2 and 3 of a one-workgroup-per-matrix complex Hermitian solve (hbatch.hip: eigx_h_batch, hgbatch.hip: eigx_hgev_batch),
// 2 NMAX threads, thread (r, hh) = (row, half): the full Hermitian matrix of order n in the split planes Ar, Ai(LD, NMAX),
// LD = NMAX + 1 -> Householder tridiagonalisation with Hermitian reflectors (the shape of EISPACK's htridi) -> a chain of unit
// phases D that makes D^H T D real with e >= 0 -> Q D accumulated in place in the planes (want_vec) -> implicit QL with Wilkinson
// shift on the real (d, e), half 0 applying the rotations to the real plane of its row and half 1 to the imaginary one.  Every
// array is the caller's LDS: d, e, hv, pr, pi, ur, ui, qr, qi of NMAX entries, pt of 4 NMAX, red[4][4], ctl[4], msk[2].  The
// caller has published the planes with a barrier; every thread of the workgroup makes the call and gets the same state back:
// ST_DONE (d holds the eigenvalues in the order of the planes' columns) or ST_FAIL (the QL budget is used up); both behind a
// barrier.
template <int NMAX>
__device__ __forceinline__ int herm_tridiag_ql(int n, int want_vec, double* Ar, double* Ai, double* d, double* e, double* hv,
                                               double* pr, double* pi, double* ur, double* ui, double* qr, double* qi, double* pt,
                                               double (*red)[4], int* ctl, unsigned long long* msk) {
  constexpr int NT = 2 * NMAX, LD = NMAX + 1;
  const int tid = threadIdx.x, r = tid % NMAX, hh = tid / NMAX;
  const bool row = hh == 0 && r < n;     // the thread that owns row r where one thread per row is wanted
  // ---- 2. tridiagonalisation, i = n-1 .. 1: H_i = I - u u^H / h annihilates A(0 .. i-2, i) and leaves g in A(i-1, i) -----
  // u stays in A(0 .. i-1, i), h in hv[i], g in (pr, pi)[i]; the active matrix is the full Hermitian block 0 .. i-1
  for (int i = n - 1; i >= 1; --i) {
    const int l = i - 1;
    double* rd = red[2 * (i & 1)];     // by parity: a step that leaves early has no closing barrier
    if (l == 0) {
      if (tid == 0) { pr[1] = Ar[LD]; pi[1] = Ai[LD]; hv[1] = 0.0; }
      continue;
    }
    const bool act = hh == 0 && r <= l;
    const double xr = act ? Ar[r + i * LD] : 0.0, xi = act ? Ai[r + i * LD] : 0.0;
    const double fr = Ar[l + i * LD], fi = Ai[l + i * LD];   // (read before the barrier: thread l overwrites them below)
    double h = block_sum<NT>(xr * xr + xi * xi, rd);
    if (h == 0.0) {                    // nothing to annihilate (uniform): the column is zero, or lost to underflow
      if (tid == 0) { pr[i] = fr; pi[i] = fi; hv[i] = 0.0; }
      continue;
    }
    const double nrm = sqrt(h), af = hypot2(fr, fi);
    double gr = -nrm, gi = 0.0;        // g = -(f / |f|) ||x||
    if (af != 0.0) {
      gr = -(fr / af) * nrm;
      gi = -(fi / af) * nrm;
    }
    h += af * nrm;                     // h = u^H u / 2
    if (act) {
      const double vr = r == l ? fr - gr : xr, vi = r == l ? fi - gi : xi;
      ur[r] = vr;
      ui[r] = vi;
      Ar[r + i * LD] = vr;
      Ai[r + i * LD] = vi;
    }
    if (tid == 0) { pr[i] = gr; pi[i] = gi; hv[i] = h; }
    __syncthreads();
    // p = A u, each half over its share of the columns.  Both halves make mid steps (a uniform trip count lets the loop be
    // unrolled and its LDS reads be batched); the step that half 1 may have too many reads column l+1 and adds nothing
    const int mid = (l + 2) / 2, k0 = hh ? mid : 0, k1 = hh ? l + 1 : mid;
    if (r <= l) {
      double sr = 0.0, si = 0.0;
#pragma unroll 4
      for (int t = 0; t < mid; ++t) {
        const int c = k0 + t;
        const double ucr = c < k1 ? ur[c] : 0.0, uci = c < k1 ? ui[c] : 0.0;
        const double ar = Ar[r + c * LD], ai = Ai[r + c * LD];
        sr = fma(ar, ucr, sr);
        sr = fma(-ai, uci, sr);
        si = fma(ar, uci, si);
        si = fma(ai, ucr, si);
      }
      pt[hh * 2 * NMAX + r] = sr;
      pt[hh * 2 * NMAX + NMAX + r] = si;
    }
    __syncthreads();
    double vr = 0.0, vi = 0.0, wr = 0.0, wi = 0.0;
    if (act) {
      vr = ur[r];
      vi = ui[r];
      wr = (pt[r] + pt[2 * NMAX + r]) / h;
      wi = (pt[NMAX + r] + pt[3 * NMAX + r]) / h;
    }
    const double hk = block_sum<NT>(vr * wr + vi * wi, rd + 4) / (h + h);   // K = u^H p / 2h (real: A is Hermitian)
    if (act) {
      qr[r] = wr - hk * vr;
      qi[r] = wi - hk * vi;
    }
    __syncthreads();
    // A <- A - u q^H - q u^H on the whole block: A(r, c) and conj(A(c, r)) are made of the same products and round alike
    if (r <= l) {
      vr = ur[r]; vi = ui[r];
      wr = qr[r]; wi = qi[r];
#pragma unroll 4
      for (int t = 0; t < mid; ++t) {
        const int c = k0 + t;
        const double ar = Ar[r + c * LD], ai = Ai[r + c * LD];
        const double qcr = qr[c], qci = qi[c], ucr = ur[c], uci = ui[c];
        const double tr = (vr * qcr + vi * qci) + (wr * ucr + wi * uci);
        const double ti = (vi * qcr - vr * qci) + (wi * ucr - wr * uci);
        if (c < k1) {
          Ar[r + c * LD] = ar - tr;
          Ai[r + c * LD] = ai - ti;
        }
      }
    }
    __syncthreads();
  }
  if (row) d[r] = Ar[r + r * LD];
  // the phases: (pr, pi)[i] = g_i -> p_i, e[i] = |conj(p_{i-1}) g_i| >= 0
  if (tid == 0) {
    e[0] = 0.0; hv[0] = 0.0;
    double cr = 1.0, ci = 0.0;
    pr[0] = 1.0; pi[0] = 0.0;
    for (int i = 1; i < n; ++i) {
      const double gr = pr[i], gi = pi[i];
      const double tr = cr * gr + ci * gi, ti = cr * gi - ci * gr;   // t = conj(p_{i-1}) g_i
      const double at = hypot2(tr, ti);
      e[i] = at;
      if (at != 0.0) { cr = tr / at; ci = -(ti / at); }
      else { cr = 1.0; ci = 0.0; }
      pr[i] = cr; pi[i] = ci;
    }
  }

  // ---- Q D, Q = H_{n-1} ... H_1 accumulated in place, i = 0 .. n-1 (tred2's second loop; column i starts as p_i e_i) -----
  if (want_vec) {
    if (r < n)
      for (int c = hh; c < r; c += 2) { Ar[r + c * LD] = 0.0; Ai[r + c * LD] = 0.0; }   // the strict lower triangle
    __syncthreads();                                         // (also publishes hv[0] and the phases)
    for (int i = 0; i < n; ++i) {
      const int l = i - 1;
      if (hh == 0 && r <= l) {
        ur[r] = Ar[r + i * LD]; ui[r] = Ai[r + i * LD];
        Ar[r + i * LD] = 0.0; Ai[r + i * LD] = 0.0;
      }
      if (hh == 0 && r == i) { Ar[i + i * LD] = pr[i]; Ai[i + i * LD] = pi[i]; }
      const double h = hv[i];
      if (l < 0 || h == 0.0) continue;                       // uniform; the next step's first barrier publishes column i
      __syncthreads();
      const int mid = (l + 2) / 2, k0 = hh ? mid : 0, k1 = hh ? l + 1 : mid;
      if (r <= l) {                                          // s = u^H Q: lane = column
        double sr = 0.0, si = 0.0;
#pragma unroll 4
        for (int t = 0; t < mid; ++t) {
          const int c = k0 + t;
          const double ucr = c < k1 ? ur[c] : 0.0, uci = c < k1 ? ui[c] : 0.0;
          const double ar = Ar[c + r * LD], ai = Ai[c + r * LD];
          sr = fma(ucr, ar, sr);
          sr = fma(uci, ai, sr);
          si = fma(ucr, ai, si);
          si = fma(-uci, ar, si);
        }
        pt[hh * 2 * NMAX + r] = sr;
        pt[hh * 2 * NMAX + NMAX + r] = si;
      }
      __syncthreads();
      if (hh == 0 && r <= l) {
        qr[r] = (pt[r] + pt[2 * NMAX + r]) / h;
        qi[r] = (pt[NMAX + r] + pt[3 * NMAX + r]) / h;
      }
      __syncthreads();
      if (r <= l) {                                          // Q <- Q - u s / h: lane = row
        const double vr = ur[r], vi = ui[r];
#pragma unroll 4
        for (int t = 0; t < mid; ++t) {
          const int c = k0 + t;
          const double ar = Ar[r + c * LD], ai = Ai[r + c * LD], scr = qr[c], sci = qi[c];
          if (c < k1) {
            Ar[r + c * LD] = fma(sci, vi, fma(-scr, vr, ar));
            Ai[r + c * LD] = fma(-sci, vr, fma(-scr, vi, ai));
          }
        }
      }
      __syncthreads();
    }
  }
  __syncthreads();

  // ---- 3. implicit QL with Wilkinson shift on (d, e) (tql2): the rounds of batch_kernel ------------------------------------
  // A round: the threads of both halves apply the rotations of the last sweep to their plane of their row of Q, the row
  // threads test every e[m] against its neighbours (one ballot per wave: bit m of msk = "e[m] is negligible"; bit n-1 is
  // always set) -> barrier -> thread 0 makes one sweep (ql_sweep) -> barrier.
  int ql_l = 0, ql_it = 0;
  if (tid == 0) {
    for (int i = 1; i < n; ++i) e[i - 1] = e[i];
    e[n - 1] = 0.0;
    ctl[0] = 0;                        // no rotations yet
    ctl[1] = 1;
    msk[1] = 0;
  }
  __syncthreads();
  for (;;) {
    {
      const int m = ctl[0], lo = ctl[1];
      if (want_vec && r < n && lo < m) {
        double* P = hh ? Ai : Ar;
        double hc = P[r + m * LD];
#pragma unroll 4
        for (int i = m - 1; i >= lo; --i) {
          const double zi = P[r + i * LD], c = pt[2 * i], s = pt[2 * i + 1];
          P[r + (i + 1) * LD] = fma(s, zi, c * hc);
          hc = fma(c, zi, -(s * hc));
        }
        P[r + lo * LD] = hc;
      }
      bool small = false;
      if (row) small = r == n - 1 || fabs(e[r]) <= (0.5 * DBL_EPSILON) * (fabs(d[r]) + fabs(d[r + 1]));
      const unsigned long long bits = __ballot(small);
      if ((tid & 63) == 0 && tid < 128) msk[tid >> 6] = bits;   // (rows live in threads 0 .. n-1; the lanes of half 1 vote 0)
    }
    __syncthreads();
    if (tid == 0) ql_sweep(n, d, e, pt, ctl, msk, ql_l, ql_it);
    __syncthreads();
    if (ctl[2] != ST_RUN) break;
  }
  return ctl[2];
}

// the place of d[r] in the ascending order of d[0 .. n-1] (rank by counting, ties by index)
__device__ inline int ascending_rank(int n, const double* d, int r) {
  const double dr = d[r];
  int rank = 0;
  for (int j = 0; j < n; ++j) {
    const double dj = d[j];
    rank += (dj < dr || (dj == dr && j < r)) ? 1 : 0;
  }
  return rank;
}

}  // namespace
}  // namespace eigx
