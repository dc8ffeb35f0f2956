// batch_common.h -- what the one-workgroup-per-matrix kernels share (batch.hip: real symmetric, hbatch.hip: complex
// Hermitian): the workgroup reductions, the failure word of a launch and the QL iteration on a real (d, e) held in LDS.
#pragma once
#include <cstdint>
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

}  // namespace
}  // namespace eigx
