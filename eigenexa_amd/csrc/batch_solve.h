// batch_solve.h -- the triangular substitutions of the one-workgroup-per-pencil kernels, one thread per column or row of the
// matrix held in LDS, against the Cholesky factor U held in LDS beside it: solve_ut / solve_u for the real kernels
// (gbatch.hip: gbatch_kernel, gvbatch.hip: gvbatch_kernel), zsolve_ut / zsolve_u on split planes for the complex one
// (hgbatch.hip: hgbatch_kernel, which serves both entries).  The uniform and the ragged entry of a family call the same
// code, so a pencil's bits do not depend on the entry that solved it.
#pragma once
#include <hip/hip_runtime.h>

// (every a*b + c that is wanted fused is written as fma())
#pragma clang fp contract(off)

namespace eigx {
namespace {

// x(0 .. n-1), entry k at x[k * inc], <- U^-T x: x_k = (x_k - sum_{j < k} U(j, k) x_j) / U(k, k), k ascending.  The sum runs
// in four interleaved chains from +0: with U = I it is +0 and x_k comes back as it was, the sign of a zero included.
template <int LD>
__device__ inline void solve_ut(int n, const double* U, double* x, int inc) {
  for (int k = 0; k < n; ++k) {
    const double* uk = U + k * LD;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int j = 0;
    for (; j + 3 < k; j += 4) {
      s0 = fma(uk[j], x[j * inc], s0);
      s1 = fma(uk[j + 1], x[(j + 1) * inc], s1);
      s2 = fma(uk[j + 2], x[(j + 2) * inc], s2);
      s3 = fma(uk[j + 3], x[(j + 3) * inc], s3);
    }
    for (; j < k; ++j) s0 = fma(uk[j], x[j * inc], s0);
    x[k * inc] = (x[k * inc] - ((s0 + s1) + (s2 + s3))) / uk[k];
  }
}
// x(0 .. n-1) <- U^-1 x: x_k = (x_k - sum_{j > k} U(k, j) x_j) / U(k, k), k descending, the sums as above
template <int LD>
__device__ inline void solve_u(int n, const double* U, double* x) {
  for (int k = n - 1; k >= 0; --k) {
    const double* uk = U + k;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int j = k + 1;
    for (; j + 3 < n; j += 4) {
      s0 = fma(uk[j * LD], x[j], s0);
      s1 = fma(uk[(j + 1) * LD], x[j + 1], s1);
      s2 = fma(uk[(j + 2) * LD], x[j + 2], s2);
      s3 = fma(uk[(j + 3) * LD], x[j + 3], s3);
    }
    for (; j < n; ++j) s0 = fma(uk[j * LD], x[j], s0);
    x[k] = (x[k] - ((s0 + s1) + (s2 + s3))) / uk[k * LD];
  }
}

// x(0 .. n-1), entry k at (xr, xi)[k * inc], <- the solution of a lower triangular system with the columns of U as rows:
// x_k = (x_k - sum_{j < k} op(U(j, k)) x_j) / U(k, k), k ascending, op = conj (CONJ: U^-H x down a column) or the identity
// (x U^-1 along a row).  The real and the imaginary sum each run in four interleaved chains from +0 (two products per term,
// two terms in flight), in an order that depends on k alone: with U = I every chain stays +0 and x_k comes back as it was, the
// sign of a zero included.  The diagonal of U is real: one division per plane.
template <int LD, bool CONJ>
__device__ inline void zsolve_ut(int n, const double* Ur, const double* Ui, double* xr, double* xi, int inc) {
  for (int k = 0; k < n; ++k) {
    const double* ukr = Ur + k * LD;
    const double* uki = Ui + k * LD;
    double r0 = 0.0, r1 = 0.0, r2 = 0.0, r3 = 0.0, i0 = 0.0, i1 = 0.0, i2 = 0.0, i3 = 0.0;
    int j = 0;
    for (; j + 1 < k; j += 2) {
      const double ar = ukr[j], at = CONJ ? -uki[j] : uki[j], br = ukr[j + 1], bt = CONJ ? -uki[j + 1] : uki[j + 1];
      const double pr = xr[j * inc], pi = xi[j * inc], qr = xr[(j + 1) * inc], qi = xi[(j + 1) * inc];
      r0 = fma(ar, pr, r0);
      r1 = fma(-at, pi, r1);
      i0 = fma(ar, pi, i0);
      i1 = fma(at, pr, i1);
      r2 = fma(br, qr, r2);
      r3 = fma(-bt, qi, r3);
      i2 = fma(br, qi, i2);
      i3 = fma(bt, qr, i3);
    }
    if (j < k) {
      const double ar = ukr[j], at = CONJ ? -uki[j] : uki[j];
      const double pr = xr[j * inc], pi = xi[j * inc];
      r0 = fma(ar, pr, r0);
      r1 = fma(-at, pi, r1);
      i0 = fma(ar, pi, i0);
      i1 = fma(at, pr, i1);
    }
    const double dk = ukr[k];
    xr[k * inc] = (xr[k * inc] - ((r0 + r1) + (r2 + r3))) / dk;
    xi[k * inc] = (xi[k * inc] - ((i0 + i1) + (i2 + i3))) / dk;
  }
}
// x(0 .. n-1) <- U^-1 x: x_k = (x_k - sum_{j > k} U(k, j) x_j) / U(k, k), k descending, the sums as above
template <int LD>
__device__ inline void zsolve_u(int n, const double* Ur, const double* Ui, double* xr, double* xi) {
  for (int k = n - 1; k >= 0; --k) {
    const double* ukr = Ur + k;
    const double* uki = Ui + k;
    double r0 = 0.0, r1 = 0.0, r2 = 0.0, r3 = 0.0, i0 = 0.0, i1 = 0.0, i2 = 0.0, i3 = 0.0;
    int j = k + 1;
    for (; j + 1 < n; j += 2) {
      const double ar = ukr[j * LD], at = uki[j * LD], br = ukr[(j + 1) * LD], bt = uki[(j + 1) * LD];
      const double pr = xr[j], pi = xi[j], qr = xr[j + 1], qi = xi[j + 1];
      r0 = fma(ar, pr, r0);
      r1 = fma(-at, pi, r1);
      i0 = fma(ar, pi, i0);
      i1 = fma(at, pr, i1);
      r2 = fma(br, qr, r2);
      r3 = fma(-bt, qi, r3);
      i2 = fma(br, qi, i2);
      i3 = fma(bt, qr, i3);
    }
    if (j < n) {
      const double ar = ukr[j * LD], at = uki[j * LD];
      const double pr = xr[j], pi = xi[j];
      r0 = fma(ar, pr, r0);
      r1 = fma(-at, pi, r1);
      i0 = fma(ar, pi, i0);
      i1 = fma(at, pr, i1);
    }
    const double dk = ukr[k * LD];
    xr[k] = (xr[k] - ((r0 + r1) + (r2 + r3))) / dk;
    xi[k] = (xi[k] - ((i0 + i1) + (i2 + i3))) / dk;
  }
}

}  // namespace
}  // namespace eigx
