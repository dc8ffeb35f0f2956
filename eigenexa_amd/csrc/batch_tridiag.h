// batch_tridiag.h -- the Householder tridiagonalisation of a windowed one-workgroup-per-matrix kernel as device functions: the
// matrix of order n held in LDS -> the real tridiagonal (d, e), the reflectors left in the matrix's columns, Q not formed.
//   sym_tridiag   real symmetric: batch_range_kernel (batch_range.hip), gbatch_range_kernel (gbatch_range.hip, on C)
//   herm_tridiag  complex Hermitian on split planes, with the chain of unit phases: hbatch_range_kernel (hbatch_range.hip),
//                 hgbatch_range_kernel (hgbatch_range.hip, on C)
// Each is the first loop of sym_tridiag_ql / herm_tridiag_ql (batch_common.h) word for word: calling these from there would move
// the code of the full-spectrum kernels (see the head of batch_common.h; DESIGN section 8h's list).  Every thread of a workgroup of
// 2 NMAX threads makes the call, thread (r, hh) = (row, half) as in batch_kernel; the results are behind a barrier.
#pragma once
#include "batch_common.h"

#pragma clang fp contract(off)

namespace eigx {
namespace {

// The full symmetric matrix of order n in A(LD, NMAX) -> (d, e), e[i] coupling i - 1 and i, e[0] = 0; the reflector of step i
// stays in A(0 .. i-1, i), its h in hv[i] (0: no reflector).
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

// The full Hermitian matrix of order n in the planes Ar, Ai(LD, NMAX) -> the real (d, e >= 0), e[i] coupling i - 1 and i,
// e[0] = 0; the reflector of step i stays in A(0 .. i-1, i), its h in hv[i] (0: no reflector), the unit phases p_i of D in
// (pr, pi)[i]: D^H (H_1 ... H_{n-1} A H_{n-1} ... H_1) D is the real tridiagonal matrix.
template <int NMAX>
__device__ __forceinline__ void herm_tridiag(int n, double* Ar, double* Ai, double* d, double* e, double* hv, double* pr, double* pi,
                                             double* ur, double* ui, double* qr, double* qi, double* pt, double (*red)[4]) {
  constexpr int NT = 2 * NMAX, LD = NMAX + 1;
  const int tid = threadIdx.x, r = tid % NMAX, hh = tid / NMAX;
  const bool row = hh == 0 && r < n;
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
  __syncthreads();
}

}  // namespace
}  // namespace eigx
