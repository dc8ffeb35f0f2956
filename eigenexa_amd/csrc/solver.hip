// solver.hip -- eigen_scaling, the solve frame and host staging (eigx_context.h), and the drivers of the standard problem:
// eigx_sx (pentadiagonal route), eigx_s (tridiagonal route) and their range solves, with their C entries.  The layout
// redistributions are in redist.hip, the generalised solvers in gev.hip (real) and hgev.hip (complex).
//
// Replaces eigen_sx (src/eigen_sx.F:30-308) and eigen_s -> eigen_FS / eigen_s0
// (src/eigen_libs.F:150-202, src/eigen_FS.F:29-300, src/eigen_s.F:30-307):
//   guards -> eigen_scaling -> band reduction -> band D&C -> back-transformation -> unscale ->
//   a(1:3,1) = flops, seconds, comm seconds (src/eigen_sx.F:285-296).
#include "eigx_context.h"
#include "eigx_comm.h"
#include "../../include/eigenexa_amd.h"
#include <algorithm>
#include <cfloat>
#include <limits>

namespace eigx {

void trbak_mg_dev(Context& ctx, int n, int nvec, const double* Aloc, int lda, double* Z, int ldz, const double* e,
                  int lde, int mb, int band);

namespace {

// max |a_ij| over the upper triangle and a non-finite flag (eigen_scaling, src/eigen_scaling.F:86-150; complex:
// src/eigen_scaling_h.F, max of |Re|, |Im|).  A is the local block of a 2-D cyclic distribution: local (i, j) = global
// (i*Px + px, j*Py + py); ncl local columns.  Im of a diagonal entry is never read (the solver ignores it throughout).
template <bool CPLX>
__global__ __launch_bounds__(256) void absmax_kernel(const double* __restrict__ A, int lda, int ncl, int Px, int px, int Py,
                                                     int py, double* __restrict__ out /* [gridDim.x][2] */) {
  constexpr int E = CPLX ? 2 : 1;   // doubles per element
  __shared__ double smax[4], sbad[4];
  double mx = 0.0, bad = 0.0;
  for (int j = blockIdx.x; j < ncl; j += gridDim.x) {
    const double* col = A + (size_t)j * lda * E;
    const int gj = j * Py + py;
    const int iend = gj >= px ? (gj - px) / Px : -1;   // last local row with global row <= gj
    for (int i = threadIdx.x; i <= iend; i += 256) {
      const double re = fabs(col[(size_t)i * E]);
      const double im = (CPLX && i * Px + px != gj) ? fabs(col[(size_t)i * E + 1]) : 0.0;
      if (!(re <= DBL_MAX) || !(im <= DBL_MAX)) bad = 1.0;
      else mx = fmax(mx, fmax(re, im));
    }
  }
  for (int o = 32; o > 0; o >>= 1) { mx = fmax(mx, __shfl_xor(mx, o, 64)); bad = fmax(bad, __shfl_xor(bad, o, 64)); }
  if ((threadIdx.x & 63) == 0) { smax[threadIdx.x >> 6] = mx; sbad[threadIdx.x >> 6] = bad; }
  __syncthreads();
  if (threadIdx.x == 0) {
    out[2 * blockIdx.x] = fmax(fmax(smax[0], smax[1]), fmax(smax[2], smax[3]));
    out[2 * blockIdx.x + 1] = fmax(fmax(sbad[0], sbad[1]), fmax(sbad[2], sbad[3]));
  }
}

__global__ void scale_upper_kernel(double* __restrict__ A, int lda, int ncl, int Px, int px, int Py, int py, double s) {
  for (int j = blockIdx.x; j < ncl; j += gridDim.x) {
    double* col = A + (size_t)j * lda;
    const int gj = j * Py + py;
    const int iend = gj >= px ? (gj - px) / Px : -1;
    for (int i = threadIdx.x; i <= iend; i += blockDim.x) col[i] *= s;
  }
}

// two-number reduction of the absmax partials on the device (so that the cross-rank MAX can follow on the stream)
__global__ void absmax_final_kernel(const double* __restrict__ part, int nb, double* __restrict__ out2) {
  __shared__ double smax[4], sbad[4];
  double mx = 0.0, bad = 0.0;
  for (int q = threadIdx.x; q < nb; q += 256) { mx = fmax(mx, part[2 * q]); bad = fmax(bad, part[2 * q + 1]); }
  for (int o = 32; o > 0; o >>= 1) { mx = fmax(mx, __shfl_xor(mx, o, 64)); bad = fmax(bad, __shfl_xor(bad, o, 64)); }
  if ((threadIdx.x & 63) == 0) { smax[threadIdx.x >> 6] = mx; sbad[threadIdx.x >> 6] = bad; }
  __syncthreads();
  if (threadIdx.x == 0) {
    out2[0] = fmax(fmax(smax[0], smax[1]), fmax(smax[2], smax[3]));
    out2[1] = fmax(fmax(sbad[0], sbad[1]), fmax(sbad[2], sbad[3]));
  }
}


// z(:, j) = e_j for the first gridDim.y columns (modes 'S', 'C': eigen_identity, src/eigen_sx.F:214)
__global__ void identity_kernel(double* __restrict__ z, int ldz, int n, int c0) {
  const int j = blockIdx.y;   // local column; global column c0 + j
  double* col = z + (size_t)j * ldz;
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) col[r] = (r == c0 + j) ? 1.0 : 0.0;
}

}  // namespace

__global__ void fill_kernel(double* p, size_t n, double v) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}
__global__ void fill_vec_kernel(double* __restrict__ w, int n, double v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) w[i] = v;
}
__global__ void scale_vec_kernel(double* __restrict__ w, int n, double s) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) w[i] *= s;
}

int eigen_scaling(Context& ctx, const double* a, int lda, bool cplx, int n, double* w, double* sigma, int nw) {
  if (nw < 0) nw = n;
  const Grid& G = ctx.grid;
  hipStream_t st = ctx.stream;
  const int nbk = 512;
  double* part = ctx.pool.get_t<double>("sol.absmax", (size_t)2 * nbk + 8);
  const int clc = local_count(n, G.Py, G.py);
  hipLaunchKernelGGL(cplx ? absmax_kernel<true> : absmax_kernel<false>, dim3(nbk), dim3(256), 0, st, a, lda, clc, G.Px, G.px,
                     G.Py, G.py, part);
  hipLaunchKernelGGL(absmax_final_kernel, dim3(1), dim3(256), 0, st, part, nbk, part + 2 * nbk);
  if (G.nranks > 1) comm_allreduce_max(ctx, COMM_WORLD, part + 2 * nbk, 2, st);       // src/eigen_scaling.F:118-123
  double hp[2] = {0.0, 0.0};
  EIGX_HIP_CHECK(hipMemcpyAsync(hp, part + 2 * nbk, sizeof(hp), hipMemcpyDeviceToHost, st));
  EIGX_HIP_CHECK(hipStreamSynchronize(st));
  if (G.nranks > 1 && comm_failed(ctx)) return EIGX_ERR_INTERNAL;
  const double anrm = hp[0], bad = hp[1];
  if (bad != 0.0) {  // NaN/Inf in the input (on any rank): w(:) = NaN on every rank (src/eigen_sx.F:151-155, src/eigen_h.F:147-150)
    if (nw > 0)   // (a count-only value-window call has no w)
      hipLaunchKernelGGL(fill_vec_kernel, dim3((nw + 255) / 256), dim3(256), 0, st, w, nw, std::numeric_limits<double>::quiet_NaN());
    EIGX_HIP_CHECK(hipStreamSynchronize(st));
    ctx.errinfo = -1;
    return EIGX_ERR_NONFINITE;
  }
  // eigen_scaling (src/eigen_scaling.F:76-81,:127-147) rescales only when max|a| leaves the safe range,
  // to RMIN/RMAX ~ 1e-146/1e+146.  This implementation forms reflector quantities that are cubic in the
  // matrix scale (u^T A u with un-normalised u), so its safe range is narrower and the target is O(1):
  // outside [1e-90, 1e90] the matrix is scaled by the exact power of two nearest to 1/max|a|.
  if (!sigma) return EIGX_OK;   // the caller only wanted the scan
  *sigma = 1.0;
  if (anrm > 0.0 && (anrm < 1e-90 || anrm > 1e90)) {
    int ex = 0;
    (void)frexp(anrm, &ex);
    *sigma = ldexp(1.0, -ex);
  }
  return EIGX_OK;
}

void* host_to_dev(Context& ctx, const char* name, const void* h, int ld, int nr, int nc, int esz) {
  const int ldd = host_ld(nr);
  void* d = ctx.pool.get(name, (size_t)esz * ldd * (nc > 0 ? nc : 1));
  if (h && nr > 0 && nc > 0)
    EIGX_HIP_CHECK(hipMemcpy2D(d, (size_t)ldd * esz, h, (size_t)ld * esz, (size_t)nr * esz, (size_t)nc, hipMemcpyHostToDevice));
  return d;
}

void dev_to_host(void* h, int ld, const void* d, int ldd, int nr, int nc, int esz) {
  if (nr > 0 && nc > 0)
    EIGX_HIP_CHECK(hipMemcpy2D(h, (size_t)ld * esz, d, (size_t)ldd * esz, (size_t)nr * esz, (size_t)nc, hipMemcpyDeviceToHost));
}

HostStage::HostStage(Context& ctx, int esz_, int nr_, int nc, const void* a_h, int lda, const void* b_h, int ldb, int zcols, int nw)
    : esz(esz_), nr(nr_), ldd(host_ld(nr_)) {
  EIGX_HIP_CHECK(hipSetDevice(ctx.device));
  const bool cx = esz == 16;
  a = (double*)host_to_dev(ctx, cx ? "host.ha" : "host.a", a_h, lda, nr, nc, esz);
  if (b_h) b = (double*)host_to_dev(ctx, cx ? "host.hb" : "host.b", b_h, ldb, nr, nc, esz);
  z = (double*)host_to_dev(ctx, cx ? "host.hz" : "host.z", nullptr, 0, nr, zcols, esz);
  w = ctx.pool.get_t<double>("host.w", (size_t)nw);
}

// ---- the solve frame (eigx_context.h) ---------------------------------------------------------------------------------
int SolveFrame::begin(bool args_ok) {
  if (!ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  if (n <= 0) {
    fprintf(stderr, "[eigx] warning: non-positive dimension is invalid\n");  // src/eigen_sx.F:95-98, src/eigen_h.F:91-94
    return EIGX_ERR_BAD_ARG;
  }
  if (!args_ok) return EIGX_ERR_BAD_ARG;
  EIGX_HIP_CHECK(hipSetDevice(ctx.device));
  // The library works on its own non-blocking streams: whatever the caller queued on the default stream to fill a
  // (a copy, a generator kernel) has to be complete before the first kernel here reads it.  (Found by a test that
  // filled `a` with an asynchronous copy and called the C-ABI directly: the second solve of a process -- workspace
  // already allocated, nothing else in the way -- overtook the copy.)
  EIGX_HIP_CHECK(hipStreamSynchronize(nullptr));
  ctx.errinfo = 0;
  ctx.dc_zero_n = 0;
  for (int q = 0; q < 16; ++q) ctx.timers[q] = 0.0;
  if (ctx.grid.nranks > 1) (void)comm_seconds(ctx, true);
  t0 = now_s();
  return EIGX_OK;
}

int SolveFrame::stage_inputs(double*& a, int& lda, double*& z, int& ldz, bool want_vec, int nvec, int nb) {
  const Grid& G = ctx.grid;
  const int P = G.nranks;
  hipStream_t st = ctx.stream;
  a_user = a;
  z_user = z;
  ldz_user = ldz;
  // The kernels read columns in 16-byte pieces: an odd leading dimension (eigen_get_matdims mode 'M' with an odd
  // ceil(n/Px) produces one) is served from an internal padded copy; `a` is destroyed by contract anyway.
  // Several GPUs: the cyclic block a(lda, *) is used IN PLACE -- nothing of A is replicated; a block-cyclic caller
  // (nb > 1, the ScaLAPACK interop entry) is converted to the cyclic layout by one all-to-all first.
  const int clr = local_count(n, G.Px, G.px), clc = local_count(n, G.Py, G.py);   // cyclic local extents
  if ((lda & 1) || ((uintptr_t)a & 15) || (P > 1 && nb > 1)) {
    const int ldi = pad_ld(clr + 2);
    double* ai = ctx.pool.get_t<double>("sol.apad", (size_t)ldi * (clc > 0 ? clc : 1));
    if (P > 1 && nb > 1) {
      const int rc_bc = bc_to_cyclic(ctx, a, lda, n, nb, ai, ldi, st);     // one all-to-all: nothing is replicated
      if (rc_bc != EIGX_OK) return rc_bc;
    } else if (clr > 0 && clc > 0) {
      EIGX_HIP_CHECK(hipMemcpy2DAsync(ai, (size_t)ldi * 8, a, (size_t)lda * 8, (size_t)clr * 8, (size_t)clc,
                                      hipMemcpyDeviceToDevice, st));
    }
    a = ai;
    lda = ldi;
  }
  // eigenvector workspace.  One GPU: the caller's z.  Several GPUs: the D&C and the back-transformation work on
  // whole eigenvector COLUMNS (rank r: columns [r*zc, (r+1)*zc) of the n x nvec matrix); the result is dealt back
  // into the caller's cyclic z(ldz, *) at the end.
  zcols = 0;
  if (P > 1 || (want_vec && ((ldz & 1) || ((uintptr_t)z & 15)))) {
    zcols = ceil_div(nvec > 0 ? nvec : 1, P);
    if (want_vec) {
      ldz = pad_ld(n);
      z = ctx.pool.get_t<double>("mg.Z", (size_t)ldz * (size_t)zcols);   // this rank's column block only
    }
  }
  return EIGX_OK;
}

void SolveFrame::return_z(const double* z, int ldz, int ncols) {
  if (z != z_user)
    EIGX_HIP_CHECK(hipMemcpy2DAsync(z_user, (size_t)ldz_user * 8, z, (size_t)ldz * 8, (size_t)n * 8, (size_t)ncols,
                                    hipMemcpyDeviceToDevice, ctx.stream));
}

int SolveFrame::scale(double* a, int lda, double* w, int nw) {
  const Grid& G = ctx.grid;
  const int rc = eigen_scaling(ctx, a, lda, cplx, n, w, &sigma, nw);
  if (rc == EIGX_OK && !cplx && sigma != 1.0)
    hipLaunchKernelGGL(scale_upper_kernel, dim3(1024), dim3(256), 0, ctx.stream, a, lda, local_count(n, G.Py, G.py), G.Px, G.px,
                       G.Py, G.py, sigma);
  return rc;
}

int SolveFrame::finish(double* w, int nw, double f_mid, int bt_cols, int stat_rows) {
  const bool peers = ctx.grid.nranks > 1;
  hipStream_t st = ctx.stream;
  if (sigma != 1.0 && sigma != 0.0 && nw > 0)
    hipLaunchKernelGGL(scale_vec_kernel, dim3((nw + 255) / 256), dim3(256), 0, st, w, nw, 1.0 / sigma);
  stage_trace(ctx.grid.rank, "exit redistribution enqueued");
  EIGX_HIP_CHECK(hipStreamSynchronize(st));
  stage_trace(ctx.grid.rank, "stream drained");
  if (peers && comm_failed(ctx)) return EIGX_ERR_INTERNAL;
  const double t4 = now_s();
  // the reference's flop model (src/eigen_sx.F:285-296, src/eigen_h.F:282-288); eigen_sx / eigen_s return it negated
  // when the middle stage counted none
  const double f_red = 4.0 / 3.0 * (double)n * n * n;
  const double f_bt = bt_cols > 0 ? 2.0 * (double)bt_cols * n * n : 0.0;
  double ret = f_red + f_mid + f_bt;
  if (!cplx && f_mid == 0.0) ret = -ret;
  // a(3,1): seconds this rank spent communicating (waits for peers included), as the reference returns; -1 on one
  // GPU, where there is none.  eigen_h has no a(3,1) and reports none (timers[4] stays 0).
  const double t_comm = (peers && !cplx) ? comm_seconds(ctx, false) : -1.0;
  ctx.timers[0] = t4 - t0; ctx.timers[1] = t2 - t1; ctx.timers[2] = t3 - t2; ctx.timers[3] = t4 - t3;
  ctx.timers[4] = (peers && !cplx) ? t_comm : 0.0; ctx.timers[12] = ret;
  // a(1:3,1) = flops, seconds, communication seconds; eigen_h: a(1,1), a(2,1) = (flops, 0), (seconds, 0)
  const double stats_r[3] = {ret, t4 - t0, t_comm}, stats_c[4] = {ret, 0.0, t4 - t0, 0.0};
  const int nst = cplx ? 2 * std::min(stat_rows, 2) : std::min(stat_rows, 3);
  if (nst > 0) EIGX_HIP_CHECK(hipMemcpyAsync(a_user, cplx ? stats_c : stats_r, (size_t)nst * 8, hipMemcpyHostToDevice, st));
  EIGX_HIP_CHECK(hipStreamSynchronize(st));
  return EIGX_OK;
}

// ---- range solve: eigenpairs il .. iu (1-based, inclusive) of the ascending spectrum, one GPU ---------------------------
// EXTENSION, not in the reference (whose nvec only trims the back-transformation, src/eigen_sx.F:200-240).
//   scaling -> band reduction (as solve_dev) -> range_window_stage (range.hip: the window, w(1:m), the band eigenvectors and
//   the early exits of a window by value) -> back-transformation of the m columns.
// w(1:m), z(:, 1:m); fill_rest (the opt-in route of eigx_sx / eigx_s, il = 1): w(m+1:n) is filled by bisection as well, so
// that w holds all n eigenvalues like the reference's.  What is sized before a window by value is resolved is sized by W.mmax.
int range_solve_dev(Context& ctx, int n, RangeWindow W, double* a, int lda, double* w, double* z, int ldz, int mf, int mb,
                    char mode, int band, bool fill_rest) {
  if (ctx.initialized && ctx.grid.nranks != 1) return refuse_several_ranks(ctx);
  mode = upper_case(mode);
  SolveFrame F(ctx, n, false);
  if (const int rc = F.begin(range_args_ok(n, W, a, lda, w, z, ldz, mode))) return rc;
  const bool want_vec = mode == 'A';
  if (mf <= 0) mf = 128;
  if (mb <= 0) mb = 128;
  hipStream_t st = ctx.stream;
  range_info_reset(W);

  if (const int rc = F.stage_inputs(a, lda, z, ldz, want_vec, W.by_value ? range_z_cap(n, W, mode) : W.m(), 1)) return rc;
  if (const int rc = F.scale(a, lda, w, fill_rest ? n : range_w_cap(W, mode))) {
    if (W.by_value) *W.m_out = 0;
    return rc;
  }

  // ---- forward reduction ---------------------------------------------------------------------------------------------
  const int lde = (n + 3) / 4 * 4;
  double* d = ctx.pool.get_t<double>("sol.d", (size_t)n);
  double* e = ctx.pool.get_t<double>("sol.e", (size_t)lde * 2);
  F.t1 = now_s();
  band_reduce_dev(ctx, n, a, lda, d, e, lde, mf, band);
  EIGX_HIP_CHECK(hipStreamSynchronize(st));
  F.t2 = now_s();

  // ---- eigenvalues il .. iu, then their band eigenvectors (range.hip): m columns go into z; the D&C's iu > m columns into
  // sub.zfull, out of which the window is copied
  const RangeStaged S = range_window_stage(F, W, mode, d, e, lde, band, w, "sub.wfull", [&](int ncols) {
    if (ncols == W.iu - W.il + 1) return RangeRoom{z, ldz};
    return RangeRoom{ctx.pool.get_t<double>("sub.zfull", (size_t)pad_ld(n) * ncols), pad_ld(n)};
  });
  if (S.ended) return S.rc;
  const int iu = W.iu, m = iu - W.il + 1;
  if (want_vec && S.z != z)
    EIGX_HIP_CHECK(hipMemcpy2DAsync(z, (size_t)ldz * 8, S.z, (size_t)S.ld * 8, (size_t)n * 8, (size_t)m, hipMemcpyDeviceToDevice, st));

  // ---- back-transformation of the m columns (prepared here: the Rayleigh-Ritz solve used the bt.* buffers) -------------
  if (want_vec) {
    trbak_dev(ctx, n, m, a, lda, z, ldz, e, lde, mb, band);
    F.return_z(z, ldz, m);
  }
  if (fill_rest && iu < n) band_bisect_range_dev(ctx, n, iu + 1, n, d, e, lde, band, w + m);
  const int rc = F.finish(w, fill_rest ? n : m, S.f_mid, want_vec ? m : 0, n);
  range_info().t[3] = ctx.timers[3];
  return rc;
}

// Host arrays.  By value: nothing is copied back into w or z on EIGX_ERR_WINDOW and on m = 0 (a non-finite input fills
// w(1:mmax) with NaN); a gets its a(1:3,1) statistics whenever the call returns EIGX_OK.
static int range_solve_host(Context& ctx, int n, RangeWindow W, double* a, int lda, double* w, double* z, int ldz, int mf, int mb,
                     char mode, int band) {
  return range_host_form(
      ctx, n, W, 8, a, lda, false, nullptr, 0, w, z, ldz, mode,
      [&](const HostStage& S) { return range_solve_dev(ctx, n, W, S.a, S.ldd, S.w, S.z, S.ldd, mf, mb, mode, band, false); },
      [&](const HostStage& S) { S.back(a, lda, S.a, 1, std::min(n, 3)); });
}

// nb = block size of the 2-D block-cyclic layout of a and z over the process grid (1 = the cyclic layout of the
// EigenExa API; a ScaLAPACK caller passes its descriptor's MB = NB and needs no pdgemr2d redistribution, manual 3.4)
int solve_dev(Context& ctx, int n, int nvec, double* a, int lda, double* w, double* z, int ldz, int mf, int mb,
              char mode, int band, int nb) {
  const Grid& G = ctx.grid;
  const int P = G.nranks;
  const int nloc_r = nb >= 1 ? numroc(n, nb, G.px, G.Px) : 0, nloc_c = nb >= 1 ? numroc(n, nb, G.py, G.Py) : 0;
  const int ld_min = nloc_r > 1 ? nloc_r : 1;
  const SolveRequest rq = normalize_request(n, nvec, mode);   // src/eigen_sx.F:108-110
  mode = rq.mode;
  nvec = rq.nvec;
  const bool want_vec = rq.want_vec;
  // opt-in (eigx_tune key 18, default off): the lowest nvec < n eigenpairs by the index-range path (EXTENSION)
  if (get_range_knob(18) == 1 && P == 1 && nb == 1 && mode == 'A' && nvec > 0 && nvec < n)
    return range_solve_dev(ctx, n, RangeWindow::index(1, nvec), a, lda, w, z, ldz, mf, mb, 'A', band, true);
  SolveFrame F(ctx, n, false);
  if (const int rc = F.begin(nb >= 1 && a && w && lda >= ld_min && (!want_vec || (z && ldz >= ld_min)))) return rc;
  if (mf <= 0) mf = 128;
  if (mb <= 0) mb = 128;
  hipStream_t st = ctx.stream;
  if (const int rc = F.stage_inputs(a, lda, z, ldz, want_vec, nvec, nb)) return rc;
  const int zcols_per_rank = F.zcols;
  if (const int rc = F.scale(a, lda, w, n)) return rc;

  // ---- forward reduction --------------------------------------------------------------------------
  const int lde = (n + 3) / 4 * 4;  // nme of src/eigen_sx.F:139
  double* d = ctx.pool.get_t<double>("sol.d", (size_t)n);
  double* e = ctx.pool.get_t<double>("sol.e", (size_t)lde * 2);
  F.t1 = now_s();
  // modes that run the D&C: zero its two Q buffers on the side stream underneath the reduction
  if (!(mode == 'N' || mode == 'S' || mode == 'C')) band_dc_prepare(ctx, n);
  band_reduce_dev(ctx, n, a, lda, d, e, lde, mf, band);
  EIGX_HIP_CHECK(hipStreamSynchronize(st));
  if (P > 1 && comm_failed(ctx)) return EIGX_ERR_INTERNAL;
  F.t2 = now_s();
  stage_trace(G.rank, "reduction done");

  // ---- divide and conquer --------------------------------------------------------------------------
  // modes (src/eigen_sx.F:200-222): A/X/T/R divide and conquer (X: eigenvalues then re-done by bisection),
  // S/C identity eigenvector matrix + bisection, N bisection only
  const bool do_bt = want_vec && mode != 'T' && mode != 'C' && mode != 'R';  // src/eigen_sx.F:240
  // The T factors of the back-transformation depend on the reflectors only: build them on the side stream while the
  // divide and conquer (launch-bound at its low levels) has the compute stream.  The reduction is complete here
  // (the host synchronised the compute stream above).
  const bool runs_dc = !(mode == 'N' || mode == 'S' || mode == 'C');
  std::function<void()> side_work;
  if (do_bt && nvec > 0 && P == 1) {
    if (runs_dc) side_work = [&ctx, n, a, lda, e, lde, mb, band] { trbak_prepare_dev(ctx, n, a, lda, e, lde, mb, band, ctx.bt_stream); };
    else trbak_prepare_dev(ctx, n, a, lda, e, lde, mb, band, ctx.side_stream);
  }
  // several GPUs: this rank's eigenvector columns [zc0, zc0 + zcnt) (the D&C delivers them, all n rows each)
  const int zc0 = (P > 1) ? ((G.rank * zcols_per_rank < nvec) ? G.rank * zcols_per_rank : nvec) : 0;
  const int zcnt = (P > 1) ? ((nvec - zc0 < zcols_per_rank) ? nvec - zc0 : zcols_per_rank) : nvec;
  if (mode == 'N' || mode == 'S' || mode == 'C') {
    if (want_vec && zcnt > 0) hipLaunchKernelGGL(identity_kernel, dim3(8, zcnt), dim3(256), 0, st, z, ldz, n, zc0);
    band_bisect_dev(ctx, n, d, e, lde, band, w);
  } else {
    band_dc_dev(ctx, n, nvec, d, e, lde, band, w, z, ldz, side_work);
    if (mode == 'X') band_bisect_dev(ctx, n, d, e, lde, band, w);
  }
  F.t3 = now_s();
  stage_trace(G.rank, "eigenvalue stage done");

  // ---- back-transformation ---------------------------------------------------------------------------
  if (do_bt) {
    if (P == 1) {
      trbak_dev(ctx, n, nvec, a, lda, z, ldz, e, lde, mb, band);
    } else {
      // eigenvector columns are split over the ranks; the reflectors stay distributed and stream past in column
      // groups (trbak.hip); no communication inside a group's sweep
      trbak_mg_dev(ctx, n, zcnt, a, lda, z, ldz, e, lde, mb, band);
    }
  }
  stage_trace(G.rank, "back-transformation enqueued");
  if (P > 1 && want_vec) cols_to_cyclic_dev(ctx, n, nvec, nb, zcols_per_rank, zc0, zcnt, z, ldz, F.z_user, F.ldz_user, st);
  else if (want_vec) F.return_z(z, ldz, nvec);
  // a(1:3,1) lives in the first local column
  return F.finish(w, n, ctx.timers[11], do_bt ? nvec : 0, nloc_c > 0 ? nloc_r : 0);
}

static int solve_host(Context& ctx, int n, int nvec, double* a, int lda, double* w, double* z, int ldz, int mf, int mb,
               char mode, int band, int nb) {
  if (!ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  if (nb < 1) return EIGX_ERR_BAD_ARG;
  const int nr = numroc(n, nb, ctx.grid.px, ctx.grid.Px), nc = numroc(n, nb, ctx.grid.py, ctx.grid.Py);
  if (n <= 0 || !a || !w || lda < nr) return EIGX_ERR_BAD_ARG;
  const HostStage S(ctx, 8, nr, nc, a, lda, nullptr, 0, nc, n);
  const int rc = solve_dev(ctx, n, nvec, S.a, S.ldd, S.w, S.z, S.ldd, mf, mb, mode, band, nb);
  S.w_back(w, n);
  if (rc != EIGX_OK) return rc;
  const SolveRequest rq = normalize_request(n, nvec, mode);
  if (z && rq.want_vec) S.back(z, ldz, S.z, numroc(rq.nvec, nb, ctx.grid.py, ctx.grid.Py));
  S.back(a, lda, S.a, 1, nc > 0 ? std::min(nr, 3) : 0);   // `a` is destroyed by contract: only the statistics
  return EIGX_OK;
}

int64_t solver_workspace_bytes(const Context& ctx, int n, int lda, int ldz, int mf, int mb) {
  (void)lda; (void)ldz;
  if (mf <= 0) mf = 128;
  if (mb <= 0) mb = 128;
  if (mf > 256) mf = 256;
  const int P = ctx.grid.nranks;
  const int64_t ldn = pad_ld(n);
  const int64_t ldp = pad_ld((n + 127) / 128 * 128 + 128);
  if (P == 1) {
    const int64_t nn = ldn * n;
    // D&C: Qa, Qb, S, S2 ; reduction: panels + partials ; back-transform: V, W, X
    return 8 * (4 * nn + (int64_t)(n + 256) * (3 * mf + 2 * (n / 128 + 2) * 2 + 8) + (int64_t)(n + 512) * mb +
                2 * (int64_t)mb * n);
  }
  // Several GPUs: everything of size n^2 is divided by P (the caller's a and z blocks are n^2/P each as well):
  //   D&C       Qa, Qb row blocks (2 n^2/P), the eigenvector-row chunk buffer (2048 n), Z column block (n^2/P),
  //   exchanges send + receive pieces of the two all-to-alls (2 n^2/P, the peer window with its growth slack),
  //   reduction replicated panels [U|W|U] + gathered panel (ldp (4 m + 2)), tile partial sums, compact panels,
  //             step window (2 P messages of 2 (nx + ny) doubles), panel-gather window,
  //   back-transformation: reflector group (2048 columns), its gather window, W / X / T / Gram blocks.
  const int64_t rp = (n + P - 1) / P, zc = rp;
  const int64_t nxs = (n + ctx.grid.Px - 1) / ctx.grid.Px + 8, nys = (n + ctx.grid.Py - 1) / ctx.grid.Py + 8;
  const int64_t maxseg = (nxs > nys ? nxs : nys) / 128 + 3;
  int64_t w = 0;
  w += 2 * (int64_t)pad_ld((int)rp + 2) * n + (int64_t)n * 2048 + ldn * zc;              // D&C + Z block
  w += (int64_t)(2.6 * (double)((nxs + 8) * ((zc / ctx.grid.Py) + 2) * P)) + 3 * rp * zc;     // the two all-to-alls
  w += (int64_t)(1.5 * (double)(rp * zc < ((int64_t)32 << 20) ? rp * zc : ((int64_t)32 << 20))) + 64;   // their bounce window
  w += ldp * (4 * mf + 2) + 2 * maxseg * 2 * ldp + 3 * ldp + (nxs + nys + 128) * 2 * mf;   // reduction panels / partials
  w += (int64_t)(1.5 * (double)(2 * P * (2 * (nxs + nys) + 8))) + (int64_t)(2.5 * (double)(P + 1) * (mf / ctx.grid.Py + 3) * nxs);
  w += (int64_t)pad_ld(n + 1024) * 2048 + (int64_t)(2.5 * (double)(P + 1) * (2048 / ctx.grid.Py + 2) * nxs);   // reflector groups
  w += 2 * (int64_t)512 * zc + 6 * (int64_t)512 * 512 * ((n + 511) / 512) / 4 + 8 * (int64_t)n;               // W, X, T, Gram
  w += (int64_t)(1.5 * 8 * 3 * n) + 16 * (int64_t)n;                                                              // small allreduces, D&C vectors
  return 8 * w;
}

}  // namespace eigx

using namespace eigx;

extern "C" {

int eigx_sx(int n, int nvec, double* a, int lda, double* w, double* z, int ldz, int mf, int mb, char mode) {
  return eigx_guard(g_ctx, [&] { return solve_host(g_ctx, n, nvec, a, lda, w, z, ldz, mf, mb, mode, 2, 1); });
}
int eigx_s(int n, int nvec, double* a, int lda, double* w, double* z, int ldz, int mf, int mb, char mode) {
  return eigx_guard(g_ctx, [&] { return solve_host(g_ctx, n, nvec, a, lda, w, z, ldz, mf, mb, mode, 1, 1); });
}
// EXTENSION: eigenpairs il .. iu of the ascending spectrum (one GPU); see range_solve_dev
int eigx_sx_range(int n, int il, int iu, double* a, int lda, double* w, double* z, int ldz, int mf, int mb, char mode) {
  return eigx_guard(g_ctx, [&] { return range_solve_host(g_ctx, n, RangeWindow::index(il, iu), a, lda, w, z, ldz, mf, mb, mode, 2); });
}
int eigx_s_range(int n, int il, int iu, double* a, int lda, double* w, double* z, int ldz, int mf, int mb, char mode) {
  return eigx_guard(g_ctx, [&] { return range_solve_host(g_ctx, n, RangeWindow::index(il, iu), a, lda, w, z, ldz, mf, mb, mode, 1); });
}
int eigx_sx_range_dev(int n, int il, int iu, double* a, int lda, double* w, double* z, int ldz, int mf, int mb, char mode) {
  return eigx_guard(g_ctx, [&] { return range_solve_dev(g_ctx, n, RangeWindow::index(il, iu), a, lda, w, z, ldz, mf, mb, mode, 2, false); });
}
int eigx_s_range_dev(int n, int il, int iu, double* a, int lda, double* w, double* z, int ldz, int mf, int mb, char mode) {
  return eigx_guard(g_ctx, [&] { return range_solve_dev(g_ctx, n, RangeWindow::index(il, iu), a, lda, w, z, ldz, mf, mb, mode, 1, false); });
}
// EXTENSION: the eigenpairs with vl <= lambda < vu (one GPU); see range_solve_dev.  m, il: host pointers in both forms
int eigx_sx_range_v(int n, double vl, double vu, int mmax, int* m, int* il, double* a, int lda, double* w, double* z, int ldz,
                    int mf, int mb, char mode) {
  return eigx_guard(g_ctx, [&] {
    return range_solve_host(g_ctx, n, RangeWindow::value(vl, vu, mmax, m, il), a, lda, w, z, ldz, mf, mb, mode, 2);
  });
}
int eigx_s_range_v(int n, double vl, double vu, int mmax, int* m, int* il, double* a, int lda, double* w, double* z, int ldz,
                   int mf, int mb, char mode) {
  return eigx_guard(g_ctx, [&] {
    return range_solve_host(g_ctx, n, RangeWindow::value(vl, vu, mmax, m, il), a, lda, w, z, ldz, mf, mb, mode, 1);
  });
}
int eigx_sx_range_v_dev(int n, double vl, double vu, int mmax, int* m, int* il, double* a, int lda, double* w, double* z,
                        int ldz, int mf, int mb, char mode) {
  return eigx_guard(g_ctx, [&] {
    return range_solve_dev(g_ctx, n, RangeWindow::value(vl, vu, mmax, m, il), a, lda, w, z, ldz, mf, mb, mode, 2, false);
  });
}
int eigx_s_range_v_dev(int n, double vl, double vu, int mmax, int* m, int* il, double* a, int lda, double* w, double* z,
                       int ldz, int mf, int mb, char mode) {
  return eigx_guard(g_ctx, [&] {
    return range_solve_dev(g_ctx, n, RangeWindow::value(vl, vu, mmax, m, il), a, lda, w, z, ldz, mf, mb, mode, 1, false);
  });
}
int eigx_sx_dev(int n, int nvec, double* a, int lda, double* w, double* z, int ldz, int mf, int mb, char mode) {
  return eigx_guard(g_ctx, [&] { return solve_dev(g_ctx, n, nvec, a, lda, w, z, ldz, mf, mb, mode, 2, 1); });
}
int eigx_s_dev(int n, int nvec, double* a, int lda, double* w, double* z, int ldz, int mf, int mb, char mode) {
  return eigx_guard(g_ctx, [&] { return solve_dev(g_ctx, n, nvec, a, lda, w, z, ldz, mf, mb, mode, 1, 1); });
}
// block-cyclic (ScaLAPACK descriptor MB = NB = nb) local blocks in and out; route 2 = eigen_sx, 1 = eigen_s
int eigx_solve_bc(int route, int n, int nvec, double* a, int lda, double* w, double* z, int ldz, int nb, int mf, int mb,
                  char mode) {
  if (route != 1 && route != 2) return EIGX_ERR_BAD_ARG;
  return eigx_guard(g_ctx, [&] { return solve_host(g_ctx, n, nvec, a, lda, w, z, ldz, mf, mb, mode, route, nb); });
}
int eigx_solve_bc_dev(int route, int n, int nvec, double* a, int lda, double* w, double* z, int ldz, int nb, int mf,
                      int mb, char mode) {
  if (route != 1 && route != 2) return EIGX_ERR_BAD_ARG;
  return eigx_guard(g_ctx, [&] { return solve_dev(g_ctx, n, nvec, a, lda, w, z, ldz, mf, mb, mode, route, nb); });
}
int eigx_numroc(int n, int nb, int iproc, int nprocs) {
  if (n < 0 || nb < 1 || nprocs < 1 || iproc < 0 || iproc >= nprocs) return -1;
  return numroc(n, nb, iproc, nprocs);
}

int eigx_band_reduce_dev(int n, double* a, int lda, double* d, double* e, int lde, int mf, int band) {
  if (!g_ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  // several ranks: collective; a = this rank's 2-D cyclic block a(lda, *), d / e replicated
  const int nloc = local_count(n, g_ctx.grid.Px, g_ctx.grid.px);
  if (n <= 0 || lda < (nloc > 1 ? nloc : 1) || (lda & 1) || lde < n || (band != 1 && band != 2)) return EIGX_ERR_BAD_ARG;
  return eigx_guard(g_ctx, [&] {
    EIGX_HIP_CHECK(hipStreamSynchronize(nullptr));   // the caller's default-stream work on the arguments (see SolveFrame::begin)
    band_reduce_dev(g_ctx, n, a, lda, d, e, lde, mf > 0 ? mf : 128, band);
    EIGX_HIP_CHECK(hipStreamSynchronize(g_ctx.stream));
    return (g_ctx.grid.nranks > 1 && comm_failed(g_ctx)) ? EIGX_ERR_INTERNAL : EIGX_OK;
  });
}

int eigx_band_dc_dev(int n, int nvec, const double* d, const double* e, int lde, int band, double* w, double* z,
                     int ldz) {
  if (!g_ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  if (n <= 0 || nvec < 0 || nvec > n || lde < n || (band != 1 && band != 2) || (nvec > 0 && ldz < n))
    return EIGX_ERR_BAD_ARG;
  if (g_ctx.grid.nranks != 1) return EIGX_ERR_INTERNAL;
  EIGX_HIP_CHECK(hipStreamSynchronize(nullptr));
  band_dc_dev(g_ctx, n, nvec, d, e, lde, band, w, z, ldz);
  return EIGX_OK;
}

int eigx_band_bisect_dev(int n, const double* d, const double* e, int lde, int band, double* w) {
  if (!g_ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  if (n <= 0 || lde < n || (band != 1 && band != 2) || !d || !e || !w) return EIGX_ERR_BAD_ARG;
  EIGX_HIP_CHECK(hipStreamSynchronize(nullptr));
  band_bisect_dev(g_ctx, n, d, e, lde, band, w);
  return EIGX_OK;
}

int eigx_trbak_dev(int n, int nvec, const double* a, int lda, double* z, int ldz, const double* e, int lde, int mb,
                   int band) {
  if (!g_ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  if (n <= 0 || nvec < 0 || lda < n || ldz < n || lde < n || (band != 1 && band != 2)) return EIGX_ERR_BAD_ARG;
  if (g_ctx.grid.nranks != 1) return EIGX_ERR_INTERNAL;
  EIGX_HIP_CHECK(hipStreamSynchronize(nullptr));
  trbak_dev(g_ctx, n, nvec, const_cast<double*>(a), lda, z, ldz, e, lde, mb > 0 ? mb : 128, band);
  EIGX_HIP_CHECK(hipStreamSynchronize(g_ctx.stream));
  return EIGX_OK;
}

}  // extern "C"
