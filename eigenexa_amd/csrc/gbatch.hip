// gbatch.hip -- eigx_gev_batch (EXTENSION, not in the reference): many small symmetric-definite pencils A x = lambda B x
// (n <= EIGX_GBATCH_NMAX) in one launch, one workgroup per pencil, both matrices resident in LDS from load to store (DESIGN
// section 8j).  The Cholesky route of eigx_gev_range inside the kernel shape of batch.hip:
//   load the upper triangles of A (mirrored) and B, scan both for NaN / Inf, scale each by a power of two (B by an even one)
//   -> B = U^T U, upper and right-looking, one column per step
//   -> C = U^-T A U^-1: a forward substitution down every column, then the same along every row; mirrored, scanned, scaled
//   -> tridiagonalisation, Q in place, implicit QL: sym_tridiag_ql of batch_common.h, the code eigx_s_batch runs
//   -> sort ascending, Z = U^-1 Y by a backward substitution down every column, unscale, store w, z and U (into b).
// No workgroup talks to another: no grid-wide barrier, no spin-wait, no atomics on the data.  Every sum is taken in an order
// that depends on n alone, so a pencil's result does not depend on its position in the batch or on the batch size.
// Pencils larger than the cutoff (eigx_tune key 23) go through gev_range_dev (gev.hip) one by one.
// Here: the kernel, the cutoff and the two functions the frame of the batch families asks for (batch_frame_dev / batch_frame_host,
// batch.hip: checks, launch and failure word, the loop above the cutoff, host staging of a, b, z, w).
#include "eigx_context.h"
#include "batch_common.h"
#include "batch_solve.h"
#include "../../include/eigenexa_amd.h"
#include <cfloat>

// (batch_common.h switches contraction off: every a*b + c that is wanted fused is written as fma())
#pragma clang fp contract(off)

namespace eigx {
namespace {

// (the substitutions solve_ut and solve_u: batch_solve.h, shared with gvbatch_kernel)

// One workgroup of 2 NMAX threads per pencil (NMAX = 32, 64, 96: the n-classes): thread (r, hh) = (row, half) as in
// batch_kernel.  S(LD, NMAX) holds A, then C, then Q, then Z; U(LD, NMAX) holds B, then its factor (upper triangle; the
// strict lower triangle is never read); column-major with LD = NMAX + 1, the access patterns of batch_kernel: lane = row at
// a fixed column is stride 1, lane = column is a stride of LD doubles, an entry of U that all lanes read is a broadcast.
template <int NMAX>
__global__ __launch_bounds__(2 * NMAX) void gbatch_kernel(int n, int batch, const double* __restrict__ a, int lda, int64_t stride_a,
                                                          double* __restrict__ b, int ldb, int64_t stride_b, double* __restrict__ w,
                                                          int ldw, double* __restrict__ z, int ldz, int64_t stride_z, int want_vec,
                                                          int* __restrict__ info, unsigned long long* __restrict__ first) {
  constexpr int NT = 2 * NMAX, LD = NMAX + 1;
  __shared__ double S[LD * NMAX];
  __shared__ double U[LD * NMAX];
  __shared__ double d[NMAX], e[NMAX], hv[NMAX], u[NMAX], q[NMAX];
  __shared__ double pt[2 * NMAX];        // the two halves' partial sums; (c_i, s_i) of a QL iteration
  __shared__ double red[4][4];           // wave partials of block_sum / block_max
  __shared__ int perm[NMAX];
  __shared__ int ctl[4];                 // QL: top index m, lowest rotation, state
  __shared__ unsigned long long msk[2];  // QL: bit m = e[m] is negligible
  const int tid = threadIdx.x, r = tid % NMAX, hh = tid / NMAX;
  const bool row = hh == 0 && r < n;     // the thread that owns row r (or column r) where one thread per row is wanted

  for (int k = blockIdx.x; k < batch; k += gridDim.x) {
    // ---- 1. load both upper triangles, mirror A, scan, scale -----------------------------------------------------------------
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
      fail_matrix(k, EIGX_ERR_NONFINITE, row, r, w, ldw, info, first);
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
    if (row) perm[r] = r;
    __syncthreads();

    // ---- 2. B = U^T U, right-looking: two barriers per column ----------------------------------------------------------------
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
      fail_matrix(k, EIGX_ERR_NOT_SPD, row, r, w, ldw, info, first);
      continue;
    }

    // ---- 3. C = U^-T A U^-1: X = U^-T A down the columns (lane = column), C = X U^-1 along the rows (lane = row) ----------------
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
      fail_matrix(k, EIGX_ERR_NOT_SPD, row, r, w, ldw, info, first);
      continue;
    }
    const int exc = scale_exponent(mxc, false);
    if (exc != 0 && r < n) {
      const double sigma = ldexp(1.0, -exc);
      for (int j = hh; j < n; j += 2) S[r + j * LD] *= sigma;
    }
    __syncthreads();

    // ---- 4. tridiagonalisation, Q in place, implicit QL (batch_common.h), sort ------------------------------------------------
    if (sym_tridiag_ql<NMAX>(n, want_vec, S, d, e, hv, u, q, pt, red, ctl, msk) == ST_FAIL) {   // uniform
      fail_matrix(k, EIGX_ERR_INTERNAL, row, r, w, ldw, info, first);
      continue;
    }
    if (row) {
      const int rank = ascending_rank(n, d, r);
      perm[rank] = r;
      w[(size_t)k * ldw + rank] = ldexp(d[r], exa - exb + exc);   // C = 2^(exb - exa - exc) times the matrix that was solved
    }
    if (tid == 0 && info) info[k] = 0;

    // ---- 5. Z = U^-1 Y down the columns (lane = column), unscale, store ---------------------------------------------------------
    if (want_vec && row) solve_u<LD>(n, U, S + r * LD);
    __syncthreads();
    if (r < n) {
      if (want_vec) {
        double* zk = z + (size_t)k * stride_z;
        for (int j = hh; j < n; j += 2) zk[r + (size_t)j * ldz] = ldexp(S[r + perm[j] * LD], -(exb / 2));
      }
      for (int j = hh; j < n; j += 2)
        if (r <= j) bk[r + (size_t)j * ldb] = ldexp(U[r + j * LD], exb / 2);
    }
    __syncthreads();
  }
}

int g_gbatch_nmax = EIGX_GBATCH_NMAX;   // key 23: largest n served by the batch kernel

void gbatch_launch(const BatchArgs& g, hipStream_t st, unsigned long long* first) {
  with_n_class<EIGX_GBATCH_NMAX>(g.n, [&](auto nmax) {
    constexpr int NMAX = decltype(nmax)::value;
    hipLaunchKernelGGL(gbatch_kernel<NMAX>, dim3((unsigned)g.batch), dim3(2 * NMAX), 0, st, g.n, g.batch, (const double*)g.a, g.lda,
                       g.stride_a, g.b, g.ldb, g.stride_b, g.w, g.ldw, g.z, g.ldz, g.stride_z, (int)(g.mode == 'A'), g.info, first);
  });
}

}  // namespace

// Above the cutoff: gev_range_dev with il = 1, iu = n.  It wants even leading dimensions: a pencil with an odd lda, ldb or ldz is
// staged through the pool buffers gbatch.a / gbatch.b / gbatch.z, and U and z are copied out where it succeeded.  The frame
// calls this once per pencil, so the three buffers are looked up by name per pencil (the same size every time: only the first
// lookup of a call can allocate).  (Also what eigx_gev_vbatch does with a block above the cutoff: gvbatch.hip.)  With a window
// il .. iu (gbatch_solve_window: eigx_gev_batch_range above the cutoff, gbatch_range.hip) w and z hold m = iu - il + 1 entries
// and columns.
int gbatch_solve_window(Context& ctx, const BatchArgs& g, int k, int il, int iu) {
  const int n = g.n, m = iu - il + 1;
  const bool want_vec = g.mode == 'A';
  double* ak = g.block(g.a, g.stride_a, k);
  double* bk = g.block(g.b, g.stride_b, k);
  double* wk = g.w + (size_t)k * g.ldw;
  double* zk = want_vec ? g.block(g.z, g.stride_z, k) : nullptr;
  const bool stage = ((g.lda | g.ldb) & 1) || (want_vec && (g.ldz & 1));
  if (!stage) return gev_range_dev(ctx, n, RangeWindow::index(il, iu), ak, g.lda, bk, g.ldb, wk, zk, g.ldz, g.mode);
  const int lds = pad_ld(n);
  const size_t col = (size_t)n * 8;
  double* as = ctx.pool.get_t<double>("gbatch.a", (size_t)lds * n);
  double* bs = ctx.pool.get_t<double>("gbatch.b", (size_t)lds * n);
  double* zs = want_vec ? ctx.pool.get_t<double>("gbatch.z", (size_t)lds * m) : nullptr;
  EIGX_HIP_CHECK(hipMemcpy2D(as, (size_t)lds * 8, ak, (size_t)g.lda * 8, col, (size_t)n, hipMemcpyDeviceToDevice));
  EIGX_HIP_CHECK(hipMemcpy2D(bs, (size_t)lds * 8, bk, (size_t)g.ldb * 8, col, (size_t)n, hipMemcpyDeviceToDevice));
  const int rk = gev_range_dev(ctx, n, RangeWindow::index(il, iu), as, lds, bs, lds, wk, zs, lds, g.mode);
  if (rk == EIGX_OK) {
    EIGX_HIP_CHECK(hipMemcpy2D(bk, (size_t)g.ldb * 8, bs, (size_t)lds * 8, col, (size_t)n, hipMemcpyDeviceToDevice));
    if (want_vec) EIGX_HIP_CHECK(hipMemcpy2D(zk, (size_t)g.ldz * 8, zs, (size_t)lds * 8, col, (size_t)m, hipMemcpyDeviceToDevice));
  }
  return rk;
}

int gbatch_solve_one(Context& ctx, const BatchArgs& g, int k) { return gbatch_solve_window(ctx, g, k, 1, g.n); }

int set_gbatch_nmax(int v) {
  if (v < 0 || v > EIGX_GBATCH_NMAX) return -1;
  const int old = g_gbatch_nmax;
  g_gbatch_nmax = v;
  return old;
}
int get_gbatch_nmax() { return g_gbatch_nmax; }

}  // namespace eigx

using namespace eigx;

extern "C" {

// EXTENSION: `batch` symmetric-definite pencils of one size (one GPU); see batch_frame_host / batch_frame_dev (batch_frame.hip)
int eigx_gev_batch(int n, int batch, double* a, int lda, int64_t stride_a, double* b, int ldb, int64_t stride_b, double* w, int ldw,
                   double* z, int ldz, int64_t stride_z, char mode, int* info) {
  const BatchArgs g{n, batch, a, lda, stride_a, b, ldb, stride_b, w, ldw, z, ldz, stride_z, mode, info, 8, true};
  return eigx_guard(g_ctx, [&] { return batch_frame_host(g_ctx, g, g_gbatch_nmax, gbatch_launch, gbatch_solve_one); });
}
int eigx_gev_batch_dev(int n, int batch, double* a_dev, int lda, int64_t stride_a, double* b_dev, int ldb, int64_t stride_b,
                       double* w_dev, int ldw, double* z_dev, int ldz, int64_t stride_z, char mode, int* info_dev) {
  const BatchArgs g{n, batch, a_dev, lda, stride_a, b_dev, ldb, stride_b, w_dev, ldw, z_dev, ldz, stride_z, mode, info_dev, 8, true};
  return eigx_guard(g_ctx, [&] { return batch_frame_dev(g_ctx, g, g_gbatch_nmax, gbatch_launch, gbatch_solve_one); });
}

}  // extern "C"
