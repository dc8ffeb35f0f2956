// hbatch.hip -- eigx_h_batch (EXTENSION, not in the reference): many small complex Hermitian eigenproblems (n <= EIGX_HBATCH_NMAX)
// in one launch, one workgroup per matrix, the matrix resident in LDS from load to store.  The complex
// sibling of batch.hip, the same kernel shape:
//   load the upper triangle (interleaved complex; of the diagonal the real parts only), mirror it with conjugation into the
//   split planes Ar, Ai, scan for NaN / Inf, scale by the rule of eigen_scaling
//   -> Householder tridiagonalisation in the shape of EISPACK's tred2 with Hermitian reflectors H = I - u u^H / h,
//      u = x - g e_l, g = -(x_l / |x_l|) ||x|| (the form of EISPACK's htridi, not LAPACK's zlarfg with a complex tau): the
//      tridiagonal matrix comes out Hermitian with the complex off-diagonal entries g
//   -> a chain of unit phases D (p_0 = 1, t = conj(p_{k-1}) g_k, e_k = |t|, p_k = conj(t) / |t|) makes D^H T D real with
//      e >= 0; Q = H_{n-1} ... H_1 is accumulated in place with p_k in place of the 1 of column k, which gives Q D
//   -> implicit QL with Wilkinson shift on the real (d, e), the sweep of batch.hip; the rotations are real, half 0 applies
//      them to the real plane of its row of Q and half 1 to the imaginary plane
//   -> sort ascending, unscale, store w(1:n), z(1:n, 1:n) interleaved.
// No workgroup talks to another: no grid-wide barrier, no spin-wait, no atomics on the data.  Every sum is taken in an order
// that depends on n alone, so a matrix's result does not depend on its position in the batch or on the batch size.
// Matrices larger than the cutoff (eigx_tune key 22) go through herm_solve_dev (eigen_h) one by one.
// Here: the kernel, the cutoff and the two functions the frame of the batch families asks for (batch_frame_dev / batch_frame_host,
// batch.hip: checks, launch and failure word, the loop above the cutoff, host staging); QL sweep and failure exit are those of batch_common.h.
#include "eigx_context.h"
#include "batch_common.h"
#include "../../include/eigenexa_amd.h"
#include <cfloat>

// (batch_common.h switches contraction off: the rank-2 update has to round A(r, c) and conj(A(c, r)) alike)
#pragma clang fp contract(off)

namespace eigx {
namespace {

// One workgroup of 2 NMAX threads per matrix (NMAX = 32, 64, 96: the n-classes): thread (r, hh) = (row, half).  The full
// Hermitian matrix, then Q, lives in the planes Ar(LD, NMAX), Ai(LD, NMAX), column-major with LD = NMAX + 1: the access
// patterns are those of batch_kernel, once per plane.  Where a loop runs over columns the two halves share it; in the
// application of the QL rotations, a chain along a row, half 0 takes the real plane and half 1 the imaginary one.
template <int NMAX>
__global__ __launch_bounds__(2 * NMAX) void hbatch_kernel(int n, int batch, const double* __restrict__ a, int lda, int64_t stride_a,
                                                          double* __restrict__ w, int ldw, double* __restrict__ z, int ldz,
                                                          int64_t stride_z, int want_vec, int* __restrict__ info,
                                                          unsigned long long* __restrict__ first) {
  constexpr int NT = 2 * NMAX, LD = NMAX + 1;
  __shared__ double Ar[LD * NMAX], Ai[LD * NMAX];
  __shared__ double d[NMAX], e[NMAX], hv[NMAX];
  __shared__ double pr[NMAX], pi[NMAX];  // the off-diagonal entries g of the Hermitian tridiagonal matrix, then the phases
  __shared__ double ur[NMAX], ui[NMAX], qr[NMAX], qi[NMAX];
  __shared__ double pt[4 * NMAX];        // the two halves' partial sums (re, im); (c_i, s_i) of a QL iteration
  __shared__ double red[4][4];           // wave partials of block_sum / block_max
  __shared__ int perm[NMAX];
  __shared__ int ctl[4];                 // QL: top index m, lowest rotation, state
  __shared__ unsigned long long msk[2];  // QL: bit m = e[m] is negligible
  const int tid = threadIdx.x, r = tid % NMAX, hh = tid / NMAX;
  const bool row = hh == 0 && r < n;     // the thread that owns row r where one thread per row is wanted

  for (int k = blockIdx.x; k < batch; k += gridDim.x) {
    // ---- 1. load the upper triangle, mirror with conjugation, scan, scale ---------------------------------------------------
    const double* ak = a + 2 * (size_t)k * stride_a;
    double mx = 0.0, bad = 0.0;
    for (int j = hh; j < n; j += 2) {
      if (r <= j) {
        const size_t at = 2 * (r + (size_t)j * lda);
        const double xr = ak[at];
        const double xi = r < j ? ak[at + 1] : 0.0;   // the imaginary part of the diagonal is not read
        if (!(fabs(xr) <= DBL_MAX) || !(fabs(xi) <= DBL_MAX)) bad = 1.0;
        else mx = fmax(mx, fmax(fabs(xr), fabs(xi)));
        Ar[r + j * LD] = xr;
        Ai[r + j * LD] = xi;
        Ar[j + r * LD] = xr;
        Ai[j + r * LD] = -xi;
      }
    }
    bad = block_max<NT>(bad, red[0]);
    mx = block_max<NT>(mx, red[1]);      // (its barrier also publishes the mirrored entries)
    if (bad != 0.0) {                    // uniform
      fail_matrix(k, EIGX_ERR_NONFINITE, row, r, w, ldw, info, first);
      continue;
    }
    // outside [1e-90, 1e90]: scale by the power of two nearest to 1 / max|a| (eigen_scaling, solver.hip)
    double unscale = 1.0;
    if (mx > 0.0 && (mx < 1e-90 || mx > 1e90)) {
      int ex = 0;
      (void)frexp(mx, &ex);
      ex = ex < -1000 ? -1000 : ex;      // (a denormal max|a|: 2^-ex has to stay finite)
      const double sigma = ldexp(1.0, -ex);
      unscale = ldexp(1.0, ex);
      if (r < n)
        for (int j = hh; j < n; j += 2) { Ar[r + j * LD] *= sigma; Ai[r + j * LD] *= sigma; }
    }
    if (row) perm[r] = r;
    __syncthreads();

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
    if (ctl[2] == ST_FAIL) {             // uniform
      fail_matrix(k, EIGX_ERR_INTERNAL, row, r, w, ldw, info, first);
      continue;
    }

    // ---- 4. sort ascending (rank by counting, ties by index), unscale, store -------------------------------------------------
    if (row) {
      const double dr = d[r];
      int rank = 0;
      for (int j = 0; j < n; ++j) {
        const double dj = d[j];
        rank += (dj < dr || (dj == dr && j < r)) ? 1 : 0;
      }
      perm[rank] = r;
      w[(size_t)k * ldw + rank] = dr * unscale;
    }
    if (tid == 0 && info) info[k] = 0;
    __syncthreads();
    if (want_vec && r < n) {
      double* zk = z + 2 * (size_t)k * stride_z;
      for (int j = hh; j < n; j += 2) {
        const int c = perm[j];
        const size_t at = 2 * (r + (size_t)j * ldz);
        zk[at] = Ar[r + c * LD];
        zk[at + 1] = Ai[r + c * LD];
      }
    }
    __syncthreads();
  }
}

int g_hbatch_nmax = EIGX_HBATCH_NMAX;   // key 22: largest n served by the batch kernel

void hbatch_launch(const BatchArgs& g, hipStream_t st, unsigned long long* first) {
  with_n_class<EIGX_HBATCH_NMAX>(g.n, [&](auto nmax) {
    constexpr int NMAX = decltype(nmax)::value;
    hipLaunchKernelGGL(hbatch_kernel<NMAX>, dim3((unsigned)g.batch), dim3(2 * NMAX), 0, st, g.n, g.batch, (const double*)g.a, g.lda,
                       g.stride_a, g.w, g.ldw, g.z, g.ldz, g.stride_z, (int)(g.mode == 'A'), g.info, first);
  });
}
// above the cutoff: eigen_h with the interface's default block sizes
int hbatch_solve_one(Context& ctx, const BatchArgs& g, int k) {
  return herm_solve_dev(ctx, g.n, g.n, g.block(g.a, g.stride_a, k), g.lda, g.w + (size_t)k * g.ldw,
                        g.mode == 'A' ? g.block(g.z, g.stride_z, k) : nullptr, g.ldz, 48, 128, g.mode);
}

}  // namespace

int set_hbatch_nmax(int v) {
  if (v < 0 || v > EIGX_HBATCH_NMAX) return -1;
  const int old = g_hbatch_nmax;
  g_hbatch_nmax = v;
  return old;
}

}  // namespace eigx

using namespace eigx;

extern "C" {

// EXTENSION: `batch` complex Hermitian eigenproblems of one size (one GPU; a, z interleaved complex; lda, ldz and the strides in
// complex elements); see batch_frame_host / batch_frame_dev (batch.hip)
int eigx_h_batch(int n, int batch, double* a, int lda, int64_t stride_a, double* w, int ldw, double* z, int ldz, int64_t stride_z,
                 char mode, int* info) {
  const BatchArgs g{n, batch, a, lda, stride_a, nullptr, 0, 0, w, ldw, z, ldz, stride_z, mode, info, 16, false};
  return eigx_guard(g_ctx, [&] { return batch_frame_host(g_ctx, g, g_hbatch_nmax, hbatch_launch, hbatch_solve_one); });
}
int eigx_h_batch_dev(int n, int batch, double* a_dev, int lda, int64_t stride_a, double* w_dev, int ldw, double* z_dev, int ldz,
                     int64_t stride_z, char mode, int* info_dev) {
  const BatchArgs g{n, batch, a_dev, lda, stride_a, nullptr, 0, 0, w_dev, ldw, z_dev, ldz, stride_z, mode, info_dev, 16, false};
  return eigx_guard(g_ctx, [&] { return batch_frame_dev(g_ctx, g, g_hbatch_nmax, hbatch_launch, hbatch_solve_one); });
}

}  // extern "C"
