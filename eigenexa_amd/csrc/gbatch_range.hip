// gbatch_range.hip -- eigx_gev_batch_range (EXTENSION, not in the reference): eigenpairs il .. iu of many small symmetric-definite
// pencils A x = lambda B x (n <= EIGX_GBATCH_NMAX) in one launch, one workgroup per pencil, both matrices resident in LDS from
// load to store.  The pencil sibling of batch_range.hip.  The window kernel (route 1):
//   load the upper triangles of A (mirrored) and B, scan, scale, B = U^T U, C = U^-T A U^-1, mirror, scan, scale: phases 1 to 3 of
//   gbatch_kernel (gbatch.hip), the same arithmetic in the same order, so U is bit for bit that entry's
//   -> Householder tridiagonalisation of C only (sym_tridiag of batch_range.hip: the reflectors stay in S's columns, Q is not formed)
//   -> the real tridiagonal window stage of batch_window.h: Sturm-count multi-section; mode 'A': inverse iteration, two passes of
//      Gram-Schmidt with the acceptance test of key 27, Rayleigh-Ritz on the m x m projection -> Y S
//   -> the n - 1 reflectors applied to its m columns (step 7 of batch_range_kernel) -> Z = U^-1 V by a backward substitution on
//      the m columns -> unscale, store w(1:m), z(1:n, 1:m) and U (into b).
// No workgroup talks to another, no atomics on the data, every sum in an order that depends on n and the window alone.  A pencil
// the acceptance test refuses leaves a mark, writes nothing (b included) and is solved again by route 2: eigx_gev_batch_dev on the
// caller's a and b (so U lands in b) with w and z in pooled workspace, and a gather of the window (bit for bit the slice of that
// entry's result).  n above the cutoff of eigx_gev_batch (eigx_tune key 23) goes through gev_range_dev pencil by pencil
// (route 3).  Which of routes 1 and 2 a call takes: eigx_tune key 26.
#include "eigx_context.h"
#include "batch_common.h"
#include "batch_solve.h"
#include "batch_window.h"
#include "../../include/eigenexa_amd.h"
#include <algorithm>
#include <cfloat>
#include <vector>

#pragma clang fp contract(off)

namespace eigx {
namespace {

// Phase 2 of sym_tridiag_ql (batch_common.h) alone: sym_tridiag of batch_range.hip word for word, which lives in that file's
// anonymous namespace (an entry on the list of DESIGN section 8h of what is written more than once).  The full symmetric matrix
// of order n in A(LD, NMAX) -> (d, e), e[i] coupling i - 1 and i, e[0] = 0; the reflector of step i stays in A(0 .. i-1, i), its h
// in hv[i] (0: no reflector).  Every thread of the workgroup makes the call; the results are behind a barrier.
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

// Route 2's second step: the window of the full solves of pencils kb .. kb + gridDim.x - 1 (rw(n, .), rz(n, n, .), rinfo: what
// eigx_gev_batch_dev left in the workspace) -> the caller's w(1:m, k), z(1:n, 1:m, k), info[k] and the first-failure word.  A
// failed pencil: w(1:m, k) = NaN, z(:, :, k) untouched.  (batch_range_gather of batch_range.hip, restated: section 8h's list.)
__global__ __launch_bounds__(256) void gbatch_range_gather(int n, int kb, int k0, int m, const double* __restrict__ rw,
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
struct GRangeBatchArgs {
  int n, batch, il, iu;
  double* a; int lda; int64_t stride_a;
  double* b; int ldb; int64_t stride_b;
  double* w; int ldw;
  double* z; int ldz; int64_t stride_z;
  char mode; int* info;
  int m() const { return iu - il + 1; }
};

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

void gbrange_launch(const GRangeBatchArgs& g, hipStream_t st, unsigned long long* first, int* redo) {
  with_n_class<EIGX_GBATCH_NMAX>(g.n, [&](auto nmax) {
    constexpr int NMAX = decltype(nmax)::value;
    constexpr int MW = NMAX <= 64 ? 16 : 0;
    hipLaunchKernelGGL((gbatch_range_kernel<NMAX, MW>), dim3((unsigned)g.batch), dim3(2 * NMAX), 0, st, g.n, g.batch, g.il - 1, g.m(),
                       (const double*)g.a, g.lda, g.stride_a, g.b, g.ldb, g.stride_b, g.w, g.ldw, g.z, g.ldz, g.stride_z,
                       (int)(g.mode == 'A'), get_batch_range_accept() / 100.0, g.info, first, redo);
  });
}

// Route 2 on pencils kb .. kb + cnt - 1: eigx_gev_batch_dev on the caller's a and b (U lands in b directly) with w and z in the
// workspace, chunk by chunk (at most 256 MiB of workspace), and the gather.  Returns EIGX_OK or a status that does not belong to
// one pencil.
int gbrange_full_and_slice(Context& ctx, const GRangeBatchArgs& g, int kb, int cnt, unsigned long long* first) {
  const int n = g.n;
  const bool want_vec = g.mode == 'A';
  const size_t per = 8 * ((size_t)n + (want_vec ? (size_t)n * n : 0));
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)cnt, ((size_t)256 << 20) / per));
  double* rw = ctx.pool.get_t<double>("gbrange.rw", (size_t)n * chunk);
  double* rz = want_vec ? ctx.pool.get_t<double>("gbrange.rz", (size_t)n * n * chunk) : nullptr;
  int* rinfo = ctx.pool.get_t<int>("gbrange.rinfo", (size_t)chunk);
  for (int c0 = 0; c0 < cnt; c0 += chunk) {
    const int nc = std::min(chunk, cnt - c0), kc = kb + c0;
    const int rc = eigx_gev_batch_dev(n, nc, g.a + (size_t)kc * g.stride_a, g.lda, g.stride_a, g.b + (size_t)kc * g.stride_b, g.ldb,
                                      g.stride_b, rw, n, rz, n, (int64_t)n * n, g.mode, rinfo);
    if (!batch_status_per_matrix(rc)) return rc;
    hipLaunchKernelGGL(gbatch_range_gather, dim3((unsigned)nc), dim3(256), 0, ctx.stream, n, kc, g.il - 1, g.m(), (const double*)rw,
                       (const double*)rz, (const int*)rinfo, g.w, g.ldw, g.z, g.ldz, g.stride_z, (int)want_vec, g.info, first);
    EIGX_HIP_CHECK(hipGetLastError());
    EIGX_HIP_CHECK(hipStreamSynchronize(ctx.stream));   // the next chunk overwrites the workspace
  }
  return EIGX_OK;
}

bool gbrange_args_ok(const GRangeBatchArgs& g) {
  const int n = g.n, batch = g.batch;
  if (n < 1 || batch < 0 || g.il < 1 || g.iu > n || g.il > g.iu || g.lda < n || g.ldb < n || g.ldw < g.m() ||
      (g.mode != 'A' && g.mode != 'N'))
    return false;
  if (batch > 1 && (g.stride_a < (int64_t)g.lda * n || g.stride_b < (int64_t)g.ldb * n)) return false;
  if (g.mode == 'A' && (g.ldz < n || (batch > 1 && g.stride_z < (int64_t)g.ldz * g.m()))) return false;
  if (batch > 0 && (!g.a || !g.b || !g.w || (g.mode == 'A' && !g.z))) return false;
  return true;
}

int gbrange_frame_dev(Context& ctx, GRangeBatchArgs g) {
  int rc;
  if (!batch_entry_begin(ctx, g.mode, g.batch, [&] { return gbrange_args_ok(g); }, rc)) return rc;
  EIGX_HIP_CHECK(hipStreamSynchronize(nullptr));   // the caller's default-stream work on the arguments
  const double t0 = now_s();
  hipStream_t st = ctx.stream;
  const int n = g.n, batch = g.batch, m = g.m();
  int redone = 0;
  if (n > get_gbatch_nmax()) {
    // route 3: the index-range solver of one large pencil (eigx_gev_range_dev; an odd leading dimension staged as eigx_gev_batch
    // does above its cutoff), pencil by pencil; errinfo is -1 after a failed pencil, as in the other windowed families (the table
    // of DESIGN section 8h)
    set_batch_range_last(3, m, 0);
    const BatchArgs u{n, batch, g.a, g.lda, g.stride_a, g.b, g.ldb, g.stride_b, g.w, g.ldw, g.z, g.ldz, g.stride_z, g.mode, g.info, 8,
                      true};
    rc = batch_loop_above_cutoff(batch, g.info, [&](int k) { return gbatch_solve_window(ctx, u, k, g.il, g.iu); });
    if (!batch_status_per_matrix(rc)) return rc;
    ctx.errinfo = rc == EIGX_OK ? 0 : -1;
  } else {
    const int key = get_batch_range_route();
    const bool eligible = g.mode == 'N' || m <= gwindow_width(n);
    const bool one = key == 2 ? false : eligible && (key == 1 || groute1_measured_faster(n, g.mode, m));
    set_batch_range_last(one ? 1 : 2, m, 0);
    FirstFailure ff;                     // a word of its own: route 2's eigx_gev_batch_dev arms batch.first while this one is live
    ff.arm(ctx, "gbrange.first", st);
    unsigned long long* first = ff.dev;
    if (one) {
      int* redo = ctx.pool.get_t<int>("gbrange.redo", (size_t)batch);
      gbrange_launch(g, st, first, redo);
      EIGX_HIP_CHECK(hipGetLastError());
      std::vector<int> marks((size_t)batch);
      EIGX_HIP_CHECK(hipMemcpyAsync(marks.data(), redo, (size_t)batch * sizeof(int), hipMemcpyDeviceToHost, st));
      EIGX_HIP_CHECK(hipStreamSynchronize(st));
      // the redo: route 2 on every run of consecutive marked pencils (route 1 left their b as it was passed: B, not U)
      for (int k = 0; k < batch;) {
        if (!marks[k]) { ++k; continue; }
        int k1 = k;
        while (k1 < batch && marks[k1]) ++k1;
        const int rr = gbrange_full_and_slice(ctx, g, k, k1 - k, first);
        if (rr != EIGX_OK) return rr;
        set_batch_range_last(1, m, redone += k1 - k);
        k = k1;
      }
    } else {
      const int rr = gbrange_full_and_slice(ctx, g, 0, batch, first);
      if (rr != EIGX_OK) return rr;
    }
    ctx.errinfo = 0;
    ff.finish(ctx, st, rc);
  }
  batch_entry_end(ctx, t0);
  return rc;
}

// Host arrays: batch_stage_host (batch_frame.hip) with has_b, m columns of z and m entries of w per pencil, in pool buffers of
// this entry's own (gbrange.h*: the names are part of the description of the entry in include/eigenexa_amd_gbatch_range.h).  b
// comes back (as U) for the pencils that succeeded.
int gbrange_frame_host(Context& ctx, GRangeBatchArgs g) {
  int rc;
  if (!batch_entry_begin(ctx, g.mode, g.batch, [&] { return gbrange_args_ok(g); }, rc)) return rc;
  const BatchArgs u{g.n, g.batch, g.a, g.lda, g.stride_a, g.b, g.ldb, g.stride_b, g.w, g.ldw, g.z, g.ldz, g.stride_z, g.mode, g.info, 8,
                    true};
  static const BatchStageNames names{"gbrange.ha", "gbrange.hb", "gbrange.hz", "gbrange.hw", "gbrange.hinfo"};
  return batch_stage_host(ctx, u, g.m(), g.m(), names, [&](const BatchArgs& dv) {
    return gbrange_frame_dev(ctx, GRangeBatchArgs{g.n, g.batch, g.il, g.iu, dv.a, dv.lda, dv.stride_a, dv.b, dv.ldb, dv.stride_b, dv.w,
                                                  dv.ldw, dv.z, dv.ldz, dv.stride_z, g.mode, dv.info});
  });
}

}  // namespace
}  // namespace eigx

using namespace eigx;

extern "C" {

// EXTENSION: eigenpairs il .. iu of `batch` symmetric-definite pencils of one size (one GPU); see gbrange_frame_host /
// gbrange_frame_dev
int eigx_gev_batch_range(int n, int batch, int il, int iu, double* a, int lda, int64_t stride_a, double* b, int ldb, int64_t stride_b,
                         double* w, int ldw, double* z, int ldz, int64_t stride_z, char mode, int* info) {
  const GRangeBatchArgs g{n, batch, il, iu, a, lda, stride_a, b, ldb, stride_b, w, ldw, z, ldz, stride_z, mode, info};
  return eigx_guard(g_ctx, [&] { return gbrange_frame_host(g_ctx, g); });
}
int eigx_gev_batch_range_dev(int n, int batch, int il, int iu, double* a_dev, int lda, int64_t stride_a, double* b_dev, int ldb,
                             int64_t stride_b, double* w_dev, int ldw, double* z_dev, int ldz, int64_t stride_z, char mode,
                             int* info_dev) {
  const GRangeBatchArgs g{n, batch, il, iu, a_dev, lda, stride_a, b_dev, ldb, stride_b, w_dev, ldw, z_dev, ldz, stride_z, mode,
                          info_dev};
  return eigx_guard(g_ctx, [&] { return gbrange_frame_dev(g_ctx, g); });
}

}  // extern "C"
