// batch_frame.hip -- the host frame of the batched entries: uniform (eigx_s_batch: batch.hip, eigx_h_batch:
// hbatch.hip, eigx_gev_batch: gbatch.hip, eigx_hgev_batch: hgbatch.hip), ragged (eigx_s_vbatch: vbatch.hip, eigx_h_vbatch:
// hvbatch.hip, eigx_gev_vbatch: gvbatch.hip, eigx_hgev_vbatch: hgbatch.hip) and windowed (eigx_s_batch_range: batch_range.hip,
// eigx_h_batch_range: hbatch_range.hip, eigx_gev_batch_range: gbatch_range.hip, eigx_hgev_batch_range: hgbatch_range.hip).
// Host code, and the one kernel that belongs to a frame and not to a family (batch_range_gather):
//   the pieces every frame is made of: the prologue (batch_entry_begin), the first-failure word (FirstFailure), the loop above
//   the cutoff of a uniform batch (batch_loop_above_cutoff), the epilogue (batch_entry_end), the host staging of a uniform batch
//   (batch_stage_host over copy_blocks);
//   the uniform frame (batch_frame_dev / batch_frame_host), the windowed frame (brange_frame_dev / brange_frame_host with
//   eigx_tune keys 26 and 27 and the record of eigx_batch_range_info) and the ragged frame (vbatch_frame_dev / vbatch_frame_host
//   with the schedule vbatch_plan) whole.
// A family supplies its kernel launch by n-class and its full-size solve of one matrix (a windowed family: its WindowFamily record);
// what errinfo is after a failed matrix differs between the frames and is tabulated in DESIGN section 8h.
#include "eigx_context.h"
#include "batch_common.h"
#include "../../include/eigenexa_amd.h"
#include <algorithm>
#include <cstdlib>
#include <vector>

namespace eigx {

// ---- the pieces ---------------------------------------------------------------------------------------------------------------
bool batch_status_per_matrix(int rc) {   // (solve_dev and herm_solve_dev never return EIGX_ERR_NOT_SPD: one set serves all)
  return rc == EIGX_OK || rc == EIGX_ERR_NONFINITE || rc == EIGX_ERR_NOT_SPD || rc == EIGX_ERR_INTERNAL;
}

bool batch_entry_begin(Context& ctx, char& mode, int batch, const std::function<bool()>& args_ok, int& rc) {
  rc = EIGX_OK;
  if (!ctx.initialized) {
    rc = EIGX_ERR_NOT_INITIALIZED;
    return false;
  }
  if (ctx.grid.nranks != 1) {
    rc = refuse_several_ranks(ctx);
    return false;
  }
  mode = upper_case(mode);
  if (!args_ok()) {
    rc = EIGX_ERR_BAD_ARG;
    return false;
  }
  if (batch == 0) return false;
  EIGX_HIP_CHECK(hipSetDevice(ctx.device));
  return true;
}

void batch_entry_end(Context& ctx, double t0) {
  for (int q = 0; q < 16; ++q) ctx.timers[q] = 0.0;
  ctx.timers[0] = now_s() - t0;
}

void FirstFailure::arm(Context& ctx, const char* name, hipStream_t st) {
  dev = ctx.pool.get_t<unsigned long long>(name, 1);
  EIGX_HIP_CHECK(hipMemsetAsync(dev, 0xff, sizeof(unsigned long long), st));
}
void FirstFailure::merge(int k, int rc) { host = std::min(host, ((unsigned long long)k << 8) | (unsigned long long)(-rc)); }
void FirstFailure::finish(Context& ctx, hipStream_t st, int& rc) {
  unsigned long long f = ~0ull;
  if (dev) EIGX_HIP_CHECK(hipMemcpyAsync(&f, dev, sizeof(f), hipMemcpyDeviceToHost, st));
  EIGX_HIP_CHECK(hipStreamSynchronize(st));
  f = std::min(f, host);
  if (f != ~0ull) {                      // (index << 8 | -code) of the failed matrix with the lowest index
    rc = -(int)(f & 0xff);
    ctx.errinfo = -1;
  }
}

int batch_loop_above_cutoff(int batch, int* info, const std::function<int(int)>& solve_one) {
  int rc = EIGX_OK;
  for (int k = 0; k < batch; ++k) {
    const int rk = solve_one(k);
    if (!batch_status_per_matrix(rk)) return rk;   // nothing per matrix: out of memory, ...
    if (info) EIGX_HIP_CHECK(hipMemcpy(info + k, &rk, sizeof(int), hipMemcpyHostToDevice));
    if (rc == EIGX_OK) rc = rk;
  }
  return rc;
}

void copy_blocks(void* dst, int ldd, int64_t sd, const void* src, int lds, int64_t ss, int nr, int nc, int b0, int nb, int esz,
                 hipMemcpyKind kind) {
  if (nb <= 0) return;
  char* d = (char*)dst;
  const char* s = (const char*)src;
  const size_t e = (size_t)esz;
  if (sd == (int64_t)ldd * nc && ss == (int64_t)lds * nc) {
    EIGX_HIP_CHECK(hipMemcpy2D(d + e * b0 * sd, e * ldd, s + e * b0 * ss, e * lds, e * nr, (size_t)nc * nb, kind));
    return;
  }
  for (int k = b0; k < b0 + nb; ++k) EIGX_HIP_CHECK(hipMemcpy2D(d + e * k * sd, e * ldd, s + e * k * ss, e * lds, e * nr, (size_t)nc, kind));
}

int batch_stage_host(Context& ctx, const BatchArgs& g, int zcols, int nw, const BatchStageNames& names,
                     const std::function<int(const BatchArgs&)>& dev_form) {
  const int n = g.n, batch = g.batch, esz = g.esz, ldd = host_ld(n);
  const bool want_vec = g.mode == 'A';
  const int64_t sd = (int64_t)ldd * n, sdz = (int64_t)ldd * zcols;
  const size_t bytes = (size_t)esz * sd * batch;
  BatchArgs dv = g;                      // the same call on the staged arrays
  dv.a = (double*)ctx.pool.get(names.a, bytes);
  dv.b = g.has_b ? (double*)ctx.pool.get(names.b, bytes) : nullptr;
  dv.z = want_vec ? (double*)ctx.pool.get(names.z, (size_t)esz * sdz * batch) : nullptr;
  dv.w = ctx.pool.get_t<double>(names.w, (size_t)nw * batch);
  dv.info = ctx.pool.get_t<int>(names.info, (size_t)batch);
  dv.lda = dv.ldb = dv.ldz = ldd;
  dv.stride_a = dv.stride_b = sd;
  dv.stride_z = sdz;
  dv.ldw = nw;
  const int64_t sa = batch > 1 ? g.stride_a : (int64_t)g.lda * n, sb = batch > 1 ? g.stride_b : (int64_t)g.ldb * n,
                sz = batch > 1 ? g.stride_z : (int64_t)g.ldz * zcols;
  copy_blocks(dv.a, ldd, sd, g.a, g.lda, sa, n, n, 0, batch, esz, hipMemcpyHostToDevice);
  if (g.has_b) copy_blocks(dv.b, ldd, sd, g.b, g.ldb, sb, n, n, 0, batch, esz, hipMemcpyHostToDevice);
  const int rc = dev_form(dv);
  if (!batch_status_per_matrix(rc)) return rc;
  std::vector<int> ih((size_t)batch);
  EIGX_HIP_CHECK(hipMemcpy(ih.data(), dv.info, (size_t)batch * sizeof(int), hipMemcpyDeviceToHost));
  EIGX_HIP_CHECK(hipMemcpy2D(g.w, (size_t)g.ldw * 8, dv.w, (size_t)nw * 8, (size_t)nw * 8, (size_t)batch, hipMemcpyDeviceToHost));
  // z and b come back in runs of matrices that succeeded (one copy_blocks per run): what the caller holds for a failed one stays
  for (int k = 0; k < batch;) {
    int k1 = k;
    while (k1 < batch && ih[k1] == EIGX_OK) ++k1;
    if (want_vec) copy_blocks(g.z, g.ldz, sz, dv.z, ldd, sdz, n, zcols, k, k1 - k, esz, hipMemcpyDeviceToHost);
    if (g.has_b) copy_blocks(g.b, g.ldb, sb, dv.b, ldd, sd, n, n, k, k1 - k, esz, hipMemcpyDeviceToHost);
    k = k1 + 1;
  }
  if (g.info) std::copy(ih.begin(), ih.end(), g.info);
  return rc;
}

// ---- the uniform frame ----------------------------------------------------------------------------------------------------------
// what both entries require of their arguments (mode in upper case)
static bool batch_args_ok(const BatchArgs& g) {
  const int n = g.n, batch = g.batch;
  if (n < 1 || batch < 0 || g.lda < n || g.ldw < n || (g.mode != 'A' && g.mode != 'N')) return false;
  if (batch > 1 && g.stride_a < (int64_t)g.lda * n) return false;
  if (g.has_b && (g.ldb < n || (batch > 1 && g.stride_b < (int64_t)g.ldb * n))) return false;
  if (g.mode == 'A' && (g.ldz < n || (batch > 1 && g.stride_z < (int64_t)g.ldz * n))) return false;
  if (batch > 0 && (!g.a || (g.has_b && !g.b) || !g.w || (g.mode == 'A' && !g.z))) return false;
  return true;
}

int batch_frame_dev(Context& ctx, BatchArgs g, int cutoff, BatchLaunch launch, BatchSolveOne solve_one) {
  int rc;
  if (!batch_entry_begin(ctx, g.mode, g.batch, [&] { return batch_args_ok(g); }, rc)) return rc;
  EIGX_HIP_CHECK(hipStreamSynchronize(nullptr));   // the caller's default-stream work on the arguments (SolveFrame::begin)
  const double t0 = now_s();
  ctx.errinfo = 0;
  if (g.n > cutoff) {
    // the full-size solver, matrix by matrix; errinfo stays 0 whatever fails here (the table of DESIGN section 8h)
    rc = batch_loop_above_cutoff(g.batch, g.info, [&](int k) { return solve_one(ctx, g, k); });
    if (!batch_status_per_matrix(rc)) return rc;
  } else {
    FirstFailure first;
    first.arm(ctx, "batch.first", ctx.stream);
    launch(g, ctx.stream, first.dev);
    EIGX_HIP_CHECK(hipGetLastError());
    first.finish(ctx, ctx.stream, rc);
  }
  batch_entry_end(ctx, t0);
  return rc;
}

// Host arrays: a, b, z and w are staged in the pool buffers of the other host forms (host.a / host.b / host.z, or host.ha / host.hb
// / host.hz at 16 bytes per element, and host.w), the per-matrix status words in batch.info.  info and w come back for every
// matrix; z (mode 'A') and b (U, every mode) for those that succeeded: a failed matrix's stay untouched.
int batch_frame_host(Context& ctx, BatchArgs g, int cutoff, BatchLaunch launch, BatchSolveOne solve_one) {
  int rc;
  if (!batch_entry_begin(ctx, g.mode, g.batch, [&] { return batch_args_ok(g); }, rc)) return rc;
  static const BatchStageNames real{"host.a", "host.b", "host.z", "host.w", "batch.info"},
      cplx{"host.ha", "host.hb", "host.hz", "host.w", "batch.info"};
  return batch_stage_host(ctx, g, g.n, g.n, g.esz == 16 ? cplx : real,
                          [&](const BatchArgs& dv) { return batch_frame_dev(ctx, dv, cutoff, launch, solve_one); });
}

// ---- the windowed frame ---------------------------------------------------------------------------------------------------------
namespace {

int g_route_key = 0;       // key 26: 0 = automatic, 1 = route 1 wherever eligible, 2 = route 2 always
int g_accept_key = 50;     // key 27: the acceptance bound in percent

// what the last call of a windowed batched entry did (eigx_batch_range_info)
struct { int route = 0, m = 0, redone = 0; } g_last;
void set_batch_range_last(int route, int m, int redone) {
  g_last.route = route;
  g_last.m = m;
  g_last.redone = redone;
}

// Route 2's second step: the window of the full solves of matrices kb .. kb + gridDim.x - 1 (rw(n, .), rz(n, n, .), rinfo: what
// the family's full_solve left in the workspace) -> the caller's w(1:m, k), z(1:n, 1:m, k), info[k] and the first-failure word.
// C doubles per element of z (2: interleaved complex, a column is 2 n doubles).  A failed matrix: w(1:m, k) = NaN, z(:, :, k)
// untouched.
template <int C>
__global__ __launch_bounds__(256) void batch_range_gather(int n, int kb, int k0, int m, const double* __restrict__ rw,
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
    // (one address; the real instance adds the two offsets one after the other, as the kernel it replaces did: the sum in
    // brackets compiles to other instructions there, profiles/brange_one_frame.log)
    const double* src = C == 1 ? rz + (size_t)kl * n * n + (size_t)k0 * n : rz + C * ((size_t)kl * n * n + (size_t)k0 * n);
    double* zk = z + C * (size_t)k * stride_z;
    for (int idx = tid; idx < C * n * m; idx += 256) zk[idx % (C * n) + C * (size_t)(idx / (C * n)) * ldz] = src[idx];
  }
  if (tid == 0 && info) info[k] = 0;
}

// Route 2 on matrices kb .. kb + cnt - 1: the family's full solve (on the caller's a, and b where there is one: U lands in b
// directly) with w and z in the workspace, chunk by chunk (at most 256 MiB of workspace), and the gather.  Returns EIGX_OK or a
// status that does not belong to one matrix.
int brange_full_and_slice(Context& ctx, const BatchArgs& g, int il, int iu, const WindowFamily& fam, int kb, int cnt,
                          unsigned long long* first) {
  const int n = g.n, m = iu - il + 1;
  const bool want_vec = g.mode == 'A';
  const size_t cs = (size_t)g.esz / 8;   // doubles per element of z
  const size_t per = 8 * ((size_t)n + (want_vec ? cs * n * n : 0));
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)cnt, ((size_t)256 << 20) / per));
  BatchArgs c = g;                       // the full solve of a chunk: the caller's a and b, the workspace's w, z and info
  c.w = ctx.pool.get_t<double>(fam.rw, (size_t)n * chunk);
  c.z = want_vec ? ctx.pool.get_t<double>(fam.rz, cs * n * n * chunk) : nullptr;
  c.info = ctx.pool.get_t<int>(fam.rinfo, (size_t)chunk);
  c.ldw = c.ldz = n;
  c.stride_z = (int64_t)n * n;
  for (int c0 = 0; c0 < cnt; c0 += chunk) {
    const int nc = std::min(chunk, cnt - c0), kc = kb + c0;
    c.batch = nc;
    c.a = g.block(g.a, g.stride_a, kc);
    if (g.has_b) c.b = g.block(g.b, g.stride_b, kc);
    const int rc = fam.full_solve(c);
    if (!batch_status_per_matrix(rc)) return rc;
    const auto gather = g.esz == 16 ? batch_range_gather<2> : batch_range_gather<1>;
    hipLaunchKernelGGL(gather, dim3((unsigned)nc), dim3(256), 0, ctx.stream, n, kc, il - 1, m, (const double*)c.w, (const double*)c.z,
                       (const int*)c.info, g.w, g.ldw, g.z, g.ldz, g.stride_z, (int)want_vec, g.info, first);
    EIGX_HIP_CHECK(hipGetLastError());
    EIGX_HIP_CHECK(hipStreamSynchronize(ctx.stream));   // the next chunk overwrites the workspace
  }
  return EIGX_OK;
}

// what the entries require of their arguments (mode in upper case)
bool brange_args_ok(const BatchArgs& g, int il, int iu) {
  const int n = g.n, batch = g.batch, m = iu - il + 1;
  if (n < 1 || batch < 0 || il < 1 || iu > n || il > iu || g.lda < n || g.ldw < m || (g.mode != 'A' && g.mode != 'N')) return false;
  if (batch > 1 && g.stride_a < (int64_t)g.lda * n) return false;
  if (g.has_b && (g.ldb < n || (batch > 1 && g.stride_b < (int64_t)g.ldb * n))) return false;
  if (g.mode == 'A' && (g.ldz < n || (batch > 1 && g.stride_z < (int64_t)g.ldz * m))) return false;
  if (batch > 0 && (!g.a || (g.has_b && !g.b) || !g.w || (g.mode == 'A' && !g.z))) return false;
  return true;
}

}  // namespace

int brange_frame_dev(Context& ctx, BatchArgs g, int il, int iu, const WindowFamily& fam) {
  int rc;
  if (!batch_entry_begin(ctx, g.mode, g.batch, [&] { return brange_args_ok(g, il, iu); }, rc)) return rc;
  EIGX_HIP_CHECK(hipStreamSynchronize(nullptr));   // the caller's default-stream work on the arguments
  const double t0 = now_s();
  hipStream_t st = ctx.stream;
  const int n = g.n, batch = g.batch, m = iu - il + 1;
  int redone = 0;
  if (n > fam.cutoff()) {
    // route 3: the family's index-range solver of one large matrix, matrix by matrix; unlike the uniform frame this one sets
    // errinfo to -1 after a failed matrix (the table of DESIGN section 8h)
    set_batch_range_last(3, m, 0);
    rc = batch_loop_above_cutoff(batch, g.info, [&](int k) { return fam.solve_window(ctx, g, k, il, iu); });
    if (!batch_status_per_matrix(rc)) return rc;
    ctx.errinfo = rc == EIGX_OK ? 0 : -1;
  } else {
    const bool eligible = g.mode == 'N' || m <= fam.window_width(n);
    const bool one = g_route_key == 2 ? false : eligible && (g_route_key == 1 || fam.route1_measured_faster(n, g.mode, m));
    set_batch_range_last(one ? 1 : 2, m, 0);
    FirstFailure ff;                     // a word of its own: route 2's full solve arms batch.first while this one is live
    ff.arm(ctx, fam.first, st);
    unsigned long long* first = ff.dev;
    if (one) {
      int* redo = ctx.pool.get_t<int>(fam.redo, (size_t)batch);
      fam.launch(g, il - 1, m, g_accept_key / 100.0, st, first, redo);
      EIGX_HIP_CHECK(hipGetLastError());
      std::vector<int> marks((size_t)batch);
      EIGX_HIP_CHECK(hipMemcpyAsync(marks.data(), redo, (size_t)batch * sizeof(int), hipMemcpyDeviceToHost, st));
      EIGX_HIP_CHECK(hipStreamSynchronize(st));
      // the redo: route 2 on every run of consecutive marked matrices (route 1 left their b as it was passed: B, not U)
      for (int k = 0; k < batch;) {
        if (!marks[k]) { ++k; continue; }
        int k1 = k;
        while (k1 < batch && marks[k1]) ++k1;
        const int rr = brange_full_and_slice(ctx, g, il, iu, fam, k, k1 - k, first);
        if (rr != EIGX_OK) return rr;
        set_batch_range_last(1, m, redone += k1 - k);
        k = k1;
      }
    } else {
      const int rr = brange_full_and_slice(ctx, g, il, iu, fam, 0, batch, first);
      if (rr != EIGX_OK) return rr;
    }
    ctx.errinfo = 0;
    ff.finish(ctx, st, rc);
  }
  batch_entry_end(ctx, t0);
  return rc;
}

// Host arrays: batch_stage_host with m columns of z and m entries of w per matrix, in pool buffers of the entry's own (fam.host:
// the names are part of the description of each entry in its public header).  b comes back (as U) for the pencils that succeeded.
int brange_frame_host(Context& ctx, BatchArgs g, int il, int iu, const WindowFamily& fam) {
  int rc;
  if (!batch_entry_begin(ctx, g.mode, g.batch, [&] { return brange_args_ok(g, il, iu); }, rc)) return rc;
  const int m = iu - il + 1;
  return batch_stage_host(ctx, g, m, m, fam.host, [&](const BatchArgs& dv) { return brange_frame_dev(ctx, dv, il, iu, fam); });
}

int set_batch_range_route(int v) {
  if (v < 0 || v > 2) return -1;
  const int old = g_route_key;
  g_route_key = v;
  return old;
}
int set_batch_range_accept(int v) {
  if (v < 0 || v > 101) return -1;
  const int old = g_accept_key;
  g_accept_key = v;
  return old;
}

// ---- the ragged frame -----------------------------------------------------------------------------------------------------------
namespace {

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
  if (!batch_entry_begin(ctx, g.mode, g.batch, [&] { return vbatch_args_ok(g); }, rc)) return rc;
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
  // the first failure of the call, as the kernels report it: the smallest (caller index << 8 | -code); a block above the cutoff
  // that failed is merged into it, so errinfo is -1 after any failed block (the table of DESIGN section 8h)
  FirstFailure first;
  // above the cutoff: the full-size solver, block by block
  std::vector<std::pair<int, int>> status;         // (k, status) of the blocks above the cutoff that failed
  for (int i = nk; i < nk + cnt[4]; ++i) {
    const int k = order[i];
    const int rk = solve_one(ctx, g, k);
    if (!batch_status_per_matrix(rk)) return rk;   // nothing per block: out of memory, ...
    if (rk != EIGX_OK) {
      status.emplace_back(k, rk);
      first.merge(k, rk);
    }
  }
  // info: 0 for every block (the empty ones and those above the cutoff included), then the failures
  if (g.info) {
    EIGX_HIP_CHECK(hipMemsetAsync(g.info, 0, (size_t)batch * sizeof(int), st));
    for (const auto& s : status) EIGX_HIP_CHECK(hipMemcpyAsync(g.info + s.first, &s.second, sizeof(int), hipMemcpyHostToDevice, st));
  }
  std::vector<Desc> desc((size_t)nk);              // (alive until the stream is drained below)
  if (nk > 0) {
    const bool want_vec = g.mode == 'A';
    const int64_t cs = g.esz / 8;                  // doubles per element of a and z
    for (int i = 0; i < nk; ++i) fill_desc(desc[i], g, order[i], want_vec, cs);
    Desc* desc_dev = ctx.pool.get_t<Desc>(desc_buffer((const Desc*)nullptr), (size_t)nk);
    EIGX_HIP_CHECK(hipMemcpyAsync(desc_dev, desc.data(), (size_t)nk * sizeof(Desc), hipMemcpyHostToDevice, st));
    first.arm(ctx, "batch.first", st);
    static const int class_n[4] = {32, 64, 96, 128};
    for (int c = 3, at = 0; c >= 0; at += cnt[c--])
      if (cnt[c] > 0) launch(class_n[c], cnt[c], desc_dev + at, g, st, first.dev);
    EIGX_HIP_CHECK(hipGetLastError());
  }
  first.finish(ctx, st, rc);
  batch_entry_end(ctx, t0);
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
  if (!batch_entry_begin(ctx, g.mode, g.batch, [&] { return vbatch_args_ok(g); }, rc)) return rc;
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

extern "C" {

// EXTENSION: what the last call of a windowed batched entry (of any of the four families) did
int eigx_batch_range_info(int* route, int* m, int* redone) {
  if (route) *route = eigx::g_last.route;
  if (m) *m = eigx::g_last.m;
  if (redone) *redone = eigx::g_last.redone;
  return EIGX_OK;
}

}  // extern "C"
