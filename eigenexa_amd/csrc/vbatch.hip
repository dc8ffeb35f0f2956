// vbatch.hip -- eigx_s_vbatch (EXTENSION, not in the reference): a ragged batch of small symmetric eigenproblems, every block with
// its own order n[k], leading dimensions and offsets into one buffer each for a, w and z.  The blocks at or
// below the cutoff (eigx_tune key 21, that of eigx_s_batch) are sorted by n-class on the host (eigx_vbatch_plan) and solved by one
// launch per non-empty class, one workgroup per block, the block resident in LDS from load to store: the phases of batch_kernel
// (batch.hip) with n, the pointers and the leading dimensions taken from the workgroup's descriptor; the reduction and the QL
// iteration are sym_tridiag_ql of batch_common.h, so a block's w and z are bit for bit those of eigx_s_batch_dev(n, 1, ...).
// No workgroup talks to another: no grid-wide barrier, no spin-wait, no atomics on the data.
// Blocks above the cutoff go through solve_dev (eigen_s) one by one; empty blocks (n = 0) are skipped.
// This file also holds the host side of every ragged family (eigx_h_vbatch: hvbatch.hip; the pencil families eigx_gev_vbatch and
// eigx_hgev_vbatch with their second matrix b: gvbatch.hip, hgvbatch.hip): the schedule, the argument check, the
// device entry (vbatch_frame_dev) and the host entry (vbatch_frame_host: staging of the spans of a, b, w and z in the pool).
#include "eigx_context.h"
#include "batch_common.h"
#include "../../include/eigenexa_amd.h"
#include <algorithm>
#include <cfloat>
#include <cstdlib>
#include <vector>

// (batch_common.h switches contraction off: the scaling and the unscaling are single products)
#pragma clang fp contract(off)

namespace eigx {
namespace {

// One workgroup of 2 NMAX threads per descriptor: thread (r, hh) = (row, half); LDS and access patterns are batch_kernel's.
template <int NMAX>
__global__ __launch_bounds__(2 * NMAX) void vbatch_kernel(const VbDesc* __restrict__ desc, const double* __restrict__ a,
                                                          double* __restrict__ w, double* __restrict__ z, int want_vec,
                                                          int* __restrict__ info, unsigned long long* __restrict__ first) {
  constexpr int NT = 2 * NMAX, LD = NMAX + 1;
  __shared__ double A[LD * NMAX];
  __shared__ double d[NMAX], e[NMAX], hv[NMAX], u[NMAX], q[NMAX];
  __shared__ double pt[2 * NMAX];        // the two halves' partial sums; (c_i, s_i) of a QL iteration
  __shared__ double red[4][4];           // wave partials of block_sum / block_max
  __shared__ int perm[NMAX];
  __shared__ int ctl[4];                 // QL: top index m, lowest rotation, state
  __shared__ unsigned long long msk[2];  // QL: bit m = e[m] is negligible
  const VbDesc ds = desc[blockIdx.x];    // uniform
  const int n = ds.n, k = ds.k, lda = ds.lda, ldz = ds.ldz;
  const int tid = threadIdx.x, r = tid % NMAX, hh = tid / NMAX;
  const bool row = hh == 0 && r < n;     // the thread that owns row r where one thread per row is wanted
  const double* ak = a + ds.off_a;
  double* wk = w + ds.off_w;

  // ---- 1. load the upper triangle, mirror, scan, scale -----------------------------------------------------------------------
  double mx = 0.0, bad = 0.0;
  for (int j = hh; j < n; j += 2) {
    if (r <= j) {
      const double x = ak[r + (size_t)j * lda];
      if (!(fabs(x) <= DBL_MAX)) bad = 1.0;
      else mx = fmax(mx, fabs(x));
      A[r + j * LD] = x;
      A[j + r * LD] = x;
    }
  }
  bad = block_max<NT>(bad, red[0]);
  mx = block_max<NT>(mx, red[1]);        // (its barrier also publishes the mirrored entries)
  if (bad != 0.0) {                      // uniform
    if (row) wk[r] = std::numeric_limits<double>::quiet_NaN();
    if (tid == 0) report_failure(first, info, k, EIGX_ERR_NONFINITE);
    return;
  }
  // outside [1e-90, 1e90]: scale by the power of two nearest to 1 / max|a| (eigen_scaling, solver.hip)
  double unscale = 1.0;
  if (mx > 0.0 && (mx < 1e-90 || mx > 1e90)) {
    int ex = 0;
    (void)frexp(mx, &ex);
    ex = ex < -1000 ? -1000 : ex;        // (a denormal max|a|: 2^-ex has to stay finite)
    const double sigma = ldexp(1.0, -ex);
    unscale = ldexp(1.0, ex);
    if (r < n)
      for (int j = hh; j < n; j += 2) A[r + j * LD] *= sigma;
  }
  if (row) perm[r] = r;
  __syncthreads();

  // ---- 2., 3. tridiagonalisation, Q in place, implicit QL (batch_common.h) -----------------------------------------------------
  if (sym_tridiag_ql<NMAX>(n, want_vec, A, d, e, hv, u, q, pt, red, ctl, msk) == ST_FAIL) {   // uniform
    if (row) wk[r] = std::numeric_limits<double>::quiet_NaN();
    if (tid == 0) report_failure(first, info, k, EIGX_ERR_INTERNAL);
    return;
  }

  // ---- 4. sort ascending (rank by counting, ties by index), unscale, store -----------------------------------------------------
  if (row) {
    const int rank = ascending_rank(n, d, r);
    perm[rank] = r;
    wk[rank] = d[r] * unscale;
  }
  if (tid == 0 && info) info[k] = 0;
  __syncthreads();
  if (want_vec && r < n) {
    double* zk = z + ds.off_z;
    for (int j = hh; j < n; j += 2) zk[r + (size_t)j * ldz] = A[r + perm[j] * LD];
  }
}

void vbatch_launch(int nclass, int count, const VbDesc* desc, const VbArgs& g, hipStream_t st, unsigned long long* first) {
  with_n_class<EIGX_BATCH_NMAX>(nclass, [&](auto nmax) {
    constexpr int NMAX = decltype(nmax)::value;
    hipLaunchKernelGGL(vbatch_kernel<NMAX>, dim3((unsigned)count), dim3(2 * NMAX), 0, st, desc, (const double*)g.a, g.w, g.z,
                       (int)(g.mode == 'A'), g.info, first);
  });
}
// above the cutoff: eigen_s with the interface's default block sizes (batch_solve_one, batch.hip)
int vbatch_solve_one(Context& ctx, const VbArgs& g, int k) {
  const int n = g.n[k];
  return solve_dev(ctx, n, n, g.a + g.off_a[k], g.lda[k], g.w + g.off_w[k], g.mode == 'A' ? g.z + g.off_z[k] : nullptr,
                   g.ldz ? g.ldz[k] : n, 48, 128, g.mode, 1, 1);
}

// the n-class of a kernel-served block as an index 0 .. 3 (32, 64, 96, 128): the rule of with_n_class
inline int class_index(int n, int top) { return n <= 32 ? 0 : n <= 64 ? 1 : (top == 96 || n <= 96) ? 2 : 3; }

// what both entries require of their arguments (mode in upper case)
bool vbatch_args_ok(const VbArgs& g) {
  const int batch = g.batch;
  const bool want_vec = g.mode == 'A';
  if (batch < 0 || (g.mode != 'A' && g.mode != 'N')) return false;
  if (batch == 0) return true;
  if (!g.n || !g.a || !g.off_a || !g.lda || !g.w || !g.off_w) return false;
  if (want_vec && (!g.z || !g.off_z || !g.ldz)) return false;
  if (g.has_b && (!g.b || !g.off_b || !g.ldb)) return false;
  for (int k = 0; k < batch; ++k) {
    const int n = g.n[k];
    if (n < 0 || g.lda[k] < n || g.off_a[k] < 0 || g.off_w[k] < 0) return false;
    if (want_vec && (g.ldz[k] < n || g.off_z[k] < 0)) return false;
    if (g.has_b && (g.ldb[k] < n || g.off_b[k] < 0)) return false;
  }
  return true;
}
// What both entries begin with (batch_begin, batch.hip).  Returns true to go on (g.mode in upper case, the device set), or false
// with the status to return in rc: a refusal, or EIGX_OK for an empty batch.
bool vbatch_begin(Context& ctx, VbArgs& g, int& rc) {
  rc = EIGX_OK;
  if (!ctx.initialized) {
    rc = EIGX_ERR_NOT_INITIALIZED;
    return false;
  }
  if (ctx.grid.nranks != 1) {
    rc = refuse_several_ranks(ctx);
    return false;
  }
  g.mode = upper_case(g.mode);
  if (!vbatch_args_ok(g)) {
    rc = EIGX_ERR_BAD_ARG;
    return false;
  }
  if (g.batch == 0) return false;
  EIGX_HIP_CHECK(hipSetDevice(ctx.device));
  return true;
}

// first element and one past the last element of the blocks of an array: block k of order n[k] > 0 covers off[k] .. off[k] +
// ld[k] (n[k] - 1) + n[k] (ld == nullptr: a vector of n[k] entries); lo = hi = 0 where every block is empty
void span_of(int batch, const int* n, const int64_t* off, const int* ld, int64_t& lo, int64_t& hi) {
  lo = INT64_MAX;
  hi = 0;
  for (int k = 0; k < batch; ++k) {
    if (n[k] == 0) continue;
    lo = std::min(lo, off[k]);
    hi = std::max(hi, off[k] + (ld ? (int64_t)ld[k] * (n[k] - 1) : 0) + n[k]);
  }
  if (lo > hi) lo = hi = 0;
}

// the descriptor of block k (cs = doubles per element of a, b and z) and the pool buffer of a call's descriptors
void fill_desc(VbDesc& d, const VbArgs& g, int k, bool want_vec, int64_t cs) {
  d = VbDesc{k, g.n[k], g.lda[k], want_vec ? g.ldz[k] : 0, cs * g.off_a[k], g.off_w[k], want_vec ? cs * g.off_z[k] : 0};
}
void fill_desc(VbPencilDesc& d, const VbArgs& g, int k, bool want_vec, int64_t cs) {
  d = VbPencilDesc{k, g.n[k], g.lda[k], g.ldb[k], want_vec ? g.ldz[k] : 0, cs * g.off_a[k], cs * g.off_b[k], g.off_w[k],
                   want_vec ? cs * g.off_z[k] : 0};
}
inline const char* desc_buffer(const VbDesc*) { return "vbatch.desc"; }
inline const char* desc_buffer(const VbPencilDesc*) { return "vbatch.pdesc"; }

}  // namespace

int vbatch_plan(int batch, const int* n, int cutoff, int top, int* order, int* counts6) {
  if (batch < 0 || (top != 96 && top != 128) || cutoff < 0 || cutoff > top) return EIGX_ERR_BAD_ARG;
  if (batch > 0 && (!n || !order)) return EIGX_ERR_BAD_ARG;
  if (!counts6) return EIGX_ERR_BAD_ARG;
  for (int k = 0; k < batch; ++k)
    if (n[k] < 0) return EIGX_ERR_BAD_ARG;
  // A class is an interval of n, so "by class from the largest down, inside a class by descending n, ties by index" is one
  // stable counting sort by descending n over the kernel-served blocks.  start[v] = first place of the blocks of order v.
  int start[EIGX_BATCH_NMAX + 2] = {0};
  int above = 0, empty = 0;
  for (int q = 0; q < 6; ++q) counts6[q] = 0;
  for (int k = 0; k < batch; ++k) {
    const int v = n[k];
    if (v == 0) ++empty;
    else if (v > cutoff) ++above;
    else {
      ++start[v];
      ++counts6[class_index(v, top)];
    }
  }
  counts6[4] = above;
  counts6[5] = empty;
  int at = 0;
  for (int v = cutoff; v >= 1; --v) {
    const int c = start[v];
    start[v] = at;
    at += c;
  }
  int at_above = at, at_empty = at + above;
  for (int k = 0; k < batch; ++k) {
    const int v = n[k];
    if (v == 0) order[at_empty++] = k;
    else if (v > cutoff) order[at_above++] = k;
    else order[start[v]++] = k;
  }
  return EIGX_OK;
}

namespace {

// the frame over the descriptor type: Desc = VbDesc (eigx_s_vbatch, eigx_h_vbatch) or VbPencilDesc (the families with has_b)
template <class Desc, class Launch>
int frame_dev(Context& ctx, VbArgs g, int cutoff, int top, Launch launch, VbSolveOne solve_one) {
  int rc;
  if (!vbatch_begin(ctx, g, rc)) return rc;
  EIGX_HIP_CHECK(hipStreamSynchronize(nullptr));   // the caller's default-stream work on the arguments (SolveFrame::begin)
  const double t0 = now_s();
  ctx.errinfo = 0;
  hipStream_t st = ctx.stream;
  const int batch = g.batch;
  std::vector<int> order((size_t)batch);
  int cnt[6];
  if (vbatch_plan(batch, g.n, std::min(cutoff, top), top, order.data(), cnt) != EIGX_OK) return EIGX_ERR_INTERNAL;
  const int nk = cnt[0] + cnt[1] + cnt[2] + cnt[3];
  // lab switch of tools/gpu_vbatch_time.py: EIGX_VBATCH_ORDER=caller keeps the caller's order inside a class
  if (const char* e = getenv("EIGX_VBATCH_ORDER"))
    if (e[0] == 'c')
      for (int c = 3, at = 0; c >= 0; at += cnt[c--]) std::sort(order.begin() + at, order.begin() + at + cnt[c]);
  // the first failure of the call, as the kernels report it: the smallest (caller index << 8 | -code)
  unsigned long long f_host = ~0ull;
  // above the cutoff: the full-size solver, block by block
  std::vector<std::pair<int, int>> status;         // (k, status) of the blocks above the cutoff that failed
  for (int i = nk; i < nk + cnt[4]; ++i) {
    const int k = order[i];
    const int rk = solve_one(ctx, g, k);
    if (!batch_status_per_matrix(rk)) return rk;   // nothing per block: out of memory, ...
    if (rk != EIGX_OK) {
      status.emplace_back(k, rk);
      f_host = std::min(f_host, ((unsigned long long)k << 8) | (unsigned long long)(-rk));
    }
  }
  // info: 0 for every block (the empty ones and those above the cutoff included), then the failures
  if (g.info) {
    EIGX_HIP_CHECK(hipMemsetAsync(g.info, 0, (size_t)batch * sizeof(int), st));
    for (const auto& s : status) EIGX_HIP_CHECK(hipMemcpyAsync(g.info + s.first, &s.second, sizeof(int), hipMemcpyHostToDevice, st));
  }
  std::vector<Desc> desc((size_t)nk);              // (alive until the stream is drained below)
  unsigned long long f = ~0ull;
  if (nk > 0) {
    const bool want_vec = g.mode == 'A';
    const int64_t cs = g.esz / 8;                  // doubles per element of a and z
    for (int i = 0; i < nk; ++i) fill_desc(desc[i], g, order[i], want_vec, cs);
    Desc* desc_dev = ctx.pool.get_t<Desc>(desc_buffer((const Desc*)nullptr), (size_t)nk);
    unsigned long long* first = ctx.pool.get_t<unsigned long long>("batch.first", 1);
    EIGX_HIP_CHECK(hipMemcpyAsync(desc_dev, desc.data(), (size_t)nk * sizeof(Desc), hipMemcpyHostToDevice, st));
    // memset 0xff of the first-failure word: all ones = "no block failed"; a failed one leaves (index << 8 | -code) by atomicMin
    EIGX_HIP_CHECK(hipMemsetAsync(first, 0xff, sizeof(unsigned long long), st));
    static const int class_n[4] = {32, 64, 96, 128};
    for (int c = 3, at = 0; c >= 0; at += cnt[c--])
      if (cnt[c] > 0) launch(class_n[c], cnt[c], desc_dev + at, g, st, first);
    EIGX_HIP_CHECK(hipGetLastError());
    EIGX_HIP_CHECK(hipMemcpyAsync(&f, first, sizeof(f), hipMemcpyDeviceToHost, st));
  }
  EIGX_HIP_CHECK(hipStreamSynchronize(st));
  f = std::min(f, f_host);
  if (f != ~0ull) {                      // (index << 8 | -code) of the failed block with the lowest caller index
    rc = -(int)(f & 0xff);
    ctx.errinfo = -1;
  }
  for (int q = 0; q < 16; ++q) ctx.timers[q] = 0.0;
  ctx.timers[0] = now_s() - t0;
  return rc;
}

// Host arrays: of each of a, w and z the span from the lowest offset to the highest last element is staged in one copy, the
// caller's layout kept and the offsets rebased, in the pool buffers of the other host forms (host.a / host.z, or host.ha / host.hz
// at 16 bytes per element, and host.w), the per-block status words in batch.info.  The spans of w and z go up before the solve
// and come back after it: gaps, padding and the z of a failed block return as they were passed.  A family with has_b: the span
// of b (host.b / host.hb) goes up before the solve and comes back after it as well, with U in the blocks that were solved.
template <class Desc, class Launch>
int frame_host(Context& ctx, VbArgs g, int cutoff, int top, Launch launch, VbSolveOne solve_one) {
  int rc;
  if (!vbatch_begin(ctx, g, rc)) return rc;
  const int batch = g.batch, esz = g.esz;
  const bool want_vec = g.mode == 'A', cplx = esz == 16;
  int64_t a0, a1, w0, w1, z0 = 0, z1 = 0, b0 = 0, b1 = 0;
  span_of(batch, g.n, g.off_a, g.lda, a0, a1);
  span_of(batch, g.n, g.off_w, nullptr, w0, w1);
  if (want_vec) span_of(batch, g.n, g.off_z, g.ldz, z0, z1);
  if (g.has_b) span_of(batch, g.n, g.off_b, g.ldb, b0, b1);
  std::vector<int64_t> oa((size_t)batch), ow((size_t)batch), oz((size_t)batch), ob((size_t)(g.has_b ? batch : 0));
  for (int k = 0; k < batch; ++k) {      // (an empty block's offsets are never used: any value that passes the check)
    const bool some = g.n[k] > 0;
    oa[k] = some ? g.off_a[k] - a0 : 0;
    ow[k] = some ? g.off_w[k] - w0 : 0;
    oz[k] = some && want_vec ? g.off_z[k] - z0 : 0;
    if (g.has_b) ob[k] = some ? g.off_b[k] - b0 : 0;
  }
  VbArgs dv = g;                         // the same call on the staged spans
  dv.a = (double*)ctx.pool.get(cplx ? "host.ha" : "host.a", (size_t)esz * std::max<int64_t>(a1 - a0, 1));
  dv.z = want_vec ? (double*)ctx.pool.get(cplx ? "host.hz" : "host.z", (size_t)esz * std::max<int64_t>(z1 - z0, 1)) : nullptr;
  dv.w = ctx.pool.get_t<double>("host.w", (size_t)std::max<int64_t>(w1 - w0, 1));
  dv.info = ctx.pool.get_t<int>("batch.info", (size_t)batch);
  dv.off_a = oa.data();
  dv.off_w = ow.data();
  dv.off_z = want_vec ? oz.data() : nullptr;
  char* bh = nullptr;
  if (g.has_b) {
    dv.b = (double*)ctx.pool.get(cplx ? "host.hb" : "host.b", (size_t)esz * std::max<int64_t>(b1 - b0, 1));
    dv.off_b = ob.data();
    bh = (char*)g.b + (size_t)esz * b0;
    if (b1 > b0) EIGX_HIP_CHECK(hipMemcpy(dv.b, bh, (size_t)esz * (b1 - b0), hipMemcpyHostToDevice));
  }
  char* ah = (char*)g.a + (size_t)esz * a0;
  char* zh = want_vec ? (char*)g.z + (size_t)esz * z0 : nullptr;
  double* wh = g.w + w0;
  if (a1 > a0) EIGX_HIP_CHECK(hipMemcpy(dv.a, ah, (size_t)esz * (a1 - a0), hipMemcpyHostToDevice));
  if (w1 > w0) EIGX_HIP_CHECK(hipMemcpy(dv.w, wh, (size_t)8 * (w1 - w0), hipMemcpyHostToDevice));
  if (z1 > z0) EIGX_HIP_CHECK(hipMemcpy(dv.z, zh, (size_t)esz * (z1 - z0), hipMemcpyHostToDevice));
  rc = frame_dev<Desc>(ctx, dv, cutoff, top, launch, solve_one);
  if (!batch_status_per_matrix(rc)) return rc;
  if (b1 > b0) EIGX_HIP_CHECK(hipMemcpy(bh, dv.b, (size_t)esz * (b1 - b0), hipMemcpyDeviceToHost));
  if (w1 > w0) EIGX_HIP_CHECK(hipMemcpy(wh, dv.w, (size_t)8 * (w1 - w0), hipMemcpyDeviceToHost));
  if (z1 > z0) EIGX_HIP_CHECK(hipMemcpy(zh, dv.z, (size_t)esz * (z1 - z0), hipMemcpyDeviceToHost));
  if (g.info) EIGX_HIP_CHECK(hipMemcpy(g.info, dv.info, (size_t)batch * sizeof(int), hipMemcpyDeviceToHost));
  return rc;
}

}  // namespace

int vbatch_frame_dev(Context& ctx, VbArgs g, int cutoff, int top, VbLaunch launch, VbSolveOne solve_one) {
  return frame_dev<VbDesc>(ctx, g, cutoff, top, launch, solve_one);
}
int vbatch_frame_host(Context& ctx, VbArgs g, int cutoff, int top, VbLaunch launch, VbSolveOne solve_one) {
  return frame_host<VbDesc>(ctx, g, cutoff, top, launch, solve_one);
}
int vbatch_frame_dev(Context& ctx, VbArgs g, int cutoff, int top, VbPencilLaunch launch, VbSolveOne solve_one) {
  return frame_dev<VbPencilDesc>(ctx, g, cutoff, top, launch, solve_one);
}
int vbatch_frame_host(Context& ctx, VbArgs g, int cutoff, int top, VbPencilLaunch launch, VbSolveOne solve_one) {
  return frame_host<VbPencilDesc>(ctx, g, cutoff, top, launch, solve_one);
}

}  // namespace eigx

using namespace eigx;

extern "C" {

// EXTENSION: the schedule of a ragged batch (pure host arithmetic; works before eigx_init and without a GPU)
int eigx_vbatch_plan(int batch, const int* n, int cutoff, int top, int* order, int* counts6) {
  return vbatch_plan(batch, n, cutoff, top, order, counts6);
}

// EXTENSION: `batch` symmetric eigenproblems of their own sizes (one GPU); see vbatch_frame_host / vbatch_frame_dev
int eigx_s_vbatch(int batch, const int* n, double* a, const int64_t* off_a, const int* lda, double* w, const int64_t* off_w, double* z,
                  const int64_t* off_z, const int* ldz, char mode, int* info) {
  const VbArgs g{batch, n, a, off_a, lda, w, off_w, z, off_z, ldz, mode, info, 8};
  return eigx_guard(g_ctx, [&] { return vbatch_frame_host(g_ctx, g, get_batch_nmax(), EIGX_BATCH_NMAX, vbatch_launch, vbatch_solve_one); });
}
int eigx_s_vbatch_dev(int batch, const int* n, double* a_dev, const int64_t* off_a, const int* lda, double* w_dev, const int64_t* off_w,
                      double* z_dev, const int64_t* off_z, const int* ldz, char mode, int* info_dev) {
  const VbArgs g{batch, n, a_dev, off_a, lda, w_dev, off_w, z_dev, off_z, ldz, mode, info_dev, 8};
  return eigx_guard(g_ctx, [&] { return vbatch_frame_dev(g_ctx, g, get_batch_nmax(), EIGX_BATCH_NMAX, vbatch_launch, vbatch_solve_one); });
}

}  // extern "C"
