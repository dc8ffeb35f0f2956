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
#include "eigx_context.h"
#include "batch_common.h"
#include "batch_window.h"
#include "../../include/eigenexa_amd.h"
#include <algorithm>
#include <cfloat>
#include <vector>

#pragma clang fp contract(off)

namespace eigx {
namespace {

// Phase 2 of herm_tridiag_ql (batch_common.h) alone, with its phase chain: the full Hermitian matrix of order n in the planes
// Ar, Ai(LD, NMAX) -> the real (d, e >= 0), e[i] coupling i - 1 and i, e[0] = 0; the reflector of step i stays in A(0 .. i-1, i),
// its h in hv[i] (0: no reflector), the unit phases p_i of D in (pr, pi)[i]: D^H (H_1 ... H_{n-1} A H_{n-1} ... H_1) D is the real
// tridiagonal matrix.  The loop is that function's first loop word for word: calling this from there would move the code of the
// existing kernels (see the head of batch_common.h).  Every thread of the workgroup makes the call; the results are behind a barrier.
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

// Route 2's second step: the window of the full solves of matrices kb .. kb + gridDim.x - 1 (rw(n, .), rz(n, n, .) interleaved
// complex, rinfo: what eigx_h_batch_dev left in the workspace) -> the caller's w(1:m, k), z(1:n, 1:m, k), info[k] and the
// first-failure word.  A failed matrix: w(1:m, k) = NaN, z(:, :, k) untouched.
__global__ __launch_bounds__(256) void hbatch_range_gather(int n, int kb, int k0, int m, const double* __restrict__ rw,
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
    const double* src = rz + 2 * ((size_t)kl * n * n + (size_t)k0 * n);   // (doubles: a column is 2 n of them)
    double* zk = z + 2 * (size_t)k * stride_z;
    for (int idx = tid; idx < 2 * n * m; idx += 256) zk[idx % (2 * n) + 2 * (size_t)(idx / (2 * n)) * ldz] = src[idx];
  }
  if (tid == 0 && info) info[k] = 0;
}

// a call: the arguments of the entries (device or host arrays; a, z interleaved complex, lda, ldz and the strides in elements)
struct HRangeBatchArgs {
  int n, batch, il, iu;
  double* a; int lda; int64_t stride_a;
  double* w; int ldw;
  double* z; int ldz; int64_t stride_z;
  char mode; int* info;
  int m() const { return iu - il + 1; }
};

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

void hbrange_launch(const HRangeBatchArgs& g, hipStream_t st, unsigned long long* first, int* redo) {
  with_n_class<EIGX_HBATCH_NMAX>(g.n, [&](auto nmax) {
    constexpr int NMAX = decltype(nmax)::value;
    constexpr int MW = NMAX <= 64 ? 16 : 0;
    hipLaunchKernelGGL((hbatch_range_kernel<NMAX, MW>), dim3((unsigned)g.batch), dim3(2 * NMAX), 0, st, g.n, g.batch, g.il - 1, g.m(),
                       (const double*)g.a, g.lda, g.stride_a, g.w, g.ldw, g.z, g.ldz, g.stride_z, (int)(g.mode == 'A'),
                       get_batch_range_accept() / 100.0, g.info, first, redo);
  });
}

// Route 2 on matrices kb .. kb + cnt - 1: eigx_h_batch_dev into the workspace, chunk by chunk (at most 256 MiB of workspace), and
// the gather.  Returns EIGX_OK or a status that does not belong to one matrix.
int hbrange_full_and_slice(Context& ctx, const HRangeBatchArgs& g, int kb, int cnt, unsigned long long* first) {
  const int n = g.n;
  const bool want_vec = g.mode == 'A';
  const size_t per = 8 * ((size_t)n + (want_vec ? 2 * (size_t)n * n : 0));
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)cnt, ((size_t)256 << 20) / per));
  double* rw = ctx.pool.get_t<double>("hbatch.rw", (size_t)n * chunk);
  double* rz = want_vec ? ctx.pool.get_t<double>("hbatch.rz", 2 * (size_t)n * n * chunk) : nullptr;
  int* rinfo = ctx.pool.get_t<int>("hbatch.rinfo", (size_t)chunk);
  for (int c0 = 0; c0 < cnt; c0 += chunk) {
    const int nc = std::min(chunk, cnt - c0), kc = kb + c0;
    const int rc = eigx_h_batch_dev(n, nc, g.a + 2 * (size_t)kc * g.stride_a, g.lda, g.stride_a, rw, n, rz, n, (int64_t)n * n, g.mode,
                                    rinfo);
    if (!batch_status_per_matrix(rc)) return rc;
    hipLaunchKernelGGL(hbatch_range_gather, dim3((unsigned)nc), dim3(256), 0, ctx.stream, n, kc, g.il - 1, g.m(), (const double*)rw,
                       (const double*)rz, (const int*)rinfo, g.w, g.ldw, g.z, g.ldz, g.stride_z, (int)want_vec, g.info, first);
    EIGX_HIP_CHECK(hipGetLastError());
    EIGX_HIP_CHECK(hipStreamSynchronize(ctx.stream));   // the next chunk overwrites the workspace
  }
  return EIGX_OK;
}

bool hbrange_args_ok(const HRangeBatchArgs& g) {
  const int n = g.n, batch = g.batch;
  if (n < 1 || batch < 0 || g.il < 1 || g.iu > n || g.il > g.iu || g.lda < n || g.ldw < g.m() || (g.mode != 'A' && g.mode != 'N'))
    return false;
  if (batch > 1 && g.stride_a < (int64_t)g.lda * n) return false;
  if (g.mode == 'A' && (g.ldz < n || (batch > 1 && g.stride_z < (int64_t)g.ldz * g.m()))) return false;
  if (batch > 0 && (!g.a || !g.w || (g.mode == 'A' && !g.z))) return false;
  return true;
}

int hbrange_frame_dev(Context& ctx, HRangeBatchArgs g) {
  int rc;
  if (!batch_entry_begin(ctx, g.mode, g.batch, [&] { return hbrange_args_ok(g); }, rc)) return rc;
  EIGX_HIP_CHECK(hipStreamSynchronize(nullptr));   // the caller's default-stream work on the arguments
  const double t0 = now_s();
  hipStream_t st = ctx.stream;
  const int n = g.n, batch = g.batch, m = g.m();
  int redone = 0;
  if (n > get_hbatch_nmax()) {
    // route 3: the index-range solver of one large matrix (eigx_h_range_dev with the interface's default block sizes), matrix by
    // matrix; errinfo is -1 after a failed matrix, as in the real family (the table of DESIGN section 8h)
    set_batch_range_last(3, m, 0);
    rc = batch_loop_above_cutoff(batch, g.info, [&](int k) {
      return herm_range_dev(ctx, n, RangeWindow::index(g.il, g.iu), g.a + 2 * (size_t)k * g.stride_a, g.lda, g.w + (size_t)k * g.ldw,
                            g.mode == 'A' ? g.z + 2 * (size_t)k * g.stride_z : nullptr, g.ldz, 48, 128, g.mode);
    });
    if (!batch_status_per_matrix(rc)) return rc;
    ctx.errinfo = rc == EIGX_OK ? 0 : -1;
  } else {
    const int key = get_batch_range_route();
    const bool eligible = g.mode == 'N' || m <= hwindow_width(n);
    const bool one = key == 2 ? false : eligible && (key == 1 || hroute1_measured_faster(n, g.mode, m));
    set_batch_range_last(one ? 1 : 2, m, 0);
    FirstFailure ff;                     // a word of its own: route 2's eigx_h_batch_dev arms batch.first while this one is live
    ff.arm(ctx, "hbrange.first", st);
    unsigned long long* first = ff.dev;
    if (one) {
      int* redo = ctx.pool.get_t<int>("hbrange.redo", (size_t)batch);
      hbrange_launch(g, st, first, redo);
      EIGX_HIP_CHECK(hipGetLastError());
      std::vector<int> marks((size_t)batch);
      EIGX_HIP_CHECK(hipMemcpyAsync(marks.data(), redo, (size_t)batch * sizeof(int), hipMemcpyDeviceToHost, st));
      EIGX_HIP_CHECK(hipStreamSynchronize(st));
      // the redo: route 2 on every run of consecutive marked matrices
      for (int k = 0; k < batch;) {
        if (!marks[k]) { ++k; continue; }
        int k1 = k;
        while (k1 < batch && marks[k1]) ++k1;
        const int rr = hbrange_full_and_slice(ctx, g, k, k1 - k, first);
        if (rr != EIGX_OK) return rr;
        set_batch_range_last(1, m, redone += k1 - k);
        k = k1;
      }
    } else {
      const int rr = hbrange_full_and_slice(ctx, g, 0, batch, first);
      if (rr != EIGX_OK) return rr;
    }
    ctx.errinfo = 0;
    ff.finish(ctx, st, rc);
  }
  batch_entry_end(ctx, t0);
  return rc;
}

// Host arrays: batch_stage_host (batch_frame.hip) with m columns of z and m entries of w per matrix at 16 bytes per element of a
// and z, in pool buffers of this entry's own (hbrange.h*: the names are part of the description of the entry in
// include/eigenexa_amd_hbatch_range.h).
int hbrange_frame_host(Context& ctx, HRangeBatchArgs g) {
  int rc;
  if (!batch_entry_begin(ctx, g.mode, g.batch, [&] { return hbrange_args_ok(g); }, rc)) return rc;
  const BatchArgs u{g.n, g.batch, g.a, g.lda, g.stride_a, nullptr, 0, 0, g.w, g.ldw, g.z, g.ldz, g.stride_z, g.mode, g.info, 16, false};
  static const BatchStageNames names{"hbrange.ha", nullptr, "hbrange.hz", "hbrange.hw", "hbrange.hinfo"};
  return batch_stage_host(ctx, u, g.m(), g.m(), names, [&](const BatchArgs& dv) {
    return hbrange_frame_dev(ctx, HRangeBatchArgs{g.n, g.batch, g.il, g.iu, dv.a, dv.lda, dv.stride_a, dv.w, dv.ldw, dv.z, dv.ldz,
                                                  dv.stride_z, g.mode, dv.info});
  });
}

}  // namespace
}  // namespace eigx

using namespace eigx;

extern "C" {

// EXTENSION: eigenpairs il .. iu of `batch` complex Hermitian matrices of one size (one GPU; a, z interleaved complex); see
// hbrange_frame_host / hbrange_frame_dev
int eigx_h_batch_range(int n, int batch, int il, int iu, double* a, int lda, int64_t stride_a, double* w, int ldw, double* z, int ldz,
                       int64_t stride_z, char mode, int* info) {
  const HRangeBatchArgs g{n, batch, il, iu, a, lda, stride_a, w, ldw, z, ldz, stride_z, mode, info};
  return eigx_guard(g_ctx, [&] { return hbrange_frame_host(g_ctx, g); });
}
int eigx_h_batch_range_dev(int n, int batch, int il, int iu, double* a_dev, int lda, int64_t stride_a, double* w_dev, int ldw,
                           double* z_dev, int ldz, int64_t stride_z, char mode, int* info_dev) {
  const HRangeBatchArgs g{n, batch, il, iu, a_dev, lda, stride_a, w_dev, ldw, z_dev, ldz, stride_z, mode, info_dev};
  return eigx_guard(g_ctx, [&] { return hbrange_frame_dev(g_ctx, g); });
}

}  // extern "C"
