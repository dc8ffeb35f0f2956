// api.hip -- C-ABI entry points (include/eigenexa_amd.h): life cycle, queries, memory helpers.
// The solver entry points live in solver.hip, gev.hip, hgev.hip, herm.hip, batch.hip, hbatch.hip, gbatch.hip and hgbatch.hip.
#include "eigx_context.h"
#include "eigx_comm.h"
#include "../../include/eigenexa_amd.h"
#include <cstring>

namespace eigx {
Context g_ctx;
}

using namespace eigx;

extern "C" {

int eigx_init(int device) {
  return eigx_init_multi(device, 0, 1, nullptr, 'C');
}

int eigx_get_device_count(void) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return ndev;
}

int eigx_get_rccl_unique_id(void* out128) {
  return comm_get_unique_id(out128);
}

// one-shot grid shape for the next eigx_init_multi (the 2-D cartesian communicator path of eigen_init,
// eigen_init_cartesian_check src/eigen_libs0.F:579-715; benchmark/main2.f:193-211 builds it for its -x option)
static int g_next_px = 0, g_next_py = 0;
int eigx_set_grid_dims(int px, int py) {
  if (px < 0 || py < 0 || (px == 0) != (py == 0)) return EIGX_ERR_BAD_ARG;
  g_next_px = px; g_next_py = py;
  return EIGX_OK;
}

int eigx_init_multi(int device, int rank, int nranks, const void* uid, char order) {
  if (g_ctx.initialized) {
    // reference behaviour: a second eigen_init self-frees first (src/eigen_libs0.F:329-339)
    fprintf(stderr, "[eigx] caution: eigx_init called twice; freeing the previous grid\n");
    eigx_free();
  }
  if (nranks < 1 || rank < 0 || rank >= nranks) return EIGX_ERR_BAD_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    fprintf(stderr, "[eigx] no HIP device visible: this library has no CPU path\n");
    return EIGX_ERR_NO_DEVICE;
  }
  if (device < 0 || device >= ndev) return EIGX_ERR_BAD_ARG;
  EIGX_HIP_CHECK(hipSetDevice(device));
  g_ctx.device = device;
  // grid rule of src/eigen_libs0.F:526-570: Px = largest divisor of P that is <= sqrt(P)
  int Px = 1;
  for (int x = 1; x * x <= nranks; ++x)
    if (nranks % x == 0) Px = x;
  int req_px = 0, req_py = 0;
  if (g_next_px > 0) {   // explicit (cartesian) shape requested
    const int rx = g_next_px, ry = g_next_py;
    req_px = rx; req_py = ry;
    g_next_px = g_next_py = 0;
    if (rx * ry != nranks) {
      fprintf(stderr, "[eigx] illegal grid dimensions %d x %d for %d ranks\n", rx, ry, nranks);
      return EIGX_ERR_BAD_ARG;
    }
    Px = rx;
  }
  // A rejected call must leave nothing behind (no streams, no half-built grid): build the grid in a local, bring up
  // the communicator first, create the streams last.
  Grid g;
  g.Px = Px;
  g.Py = nranks / Px;
  g.rank = rank;
  g.nranks = nranks;
  if (order == 'R' || order == 'r') {  // row-major rank order (src/eigen_libs0.F:2336-2356)
    g.px = rank / g.Py;
    g.py = rank % g.Py;
    g.row_major = 1;
  } else {
    g.px = rank % g.Px;
    g.py = rank / g.Px;
    g.row_major = 0;
  }
  g_ctx.grid = g;
  if (nranks > 1) {
    const int rc = comm_init(g_ctx, uid);
    if (rc != 0) {   // nothing was created; a requested grid shape stays pending for the retry
      g_ctx.grid = Grid();
      g_next_px = req_px; g_next_py = req_py;
      return rc;
    }
  }
  EIGX_HIP_CHECK(hipStreamCreateWithFlags(&g_ctx.stream, hipStreamNonBlocking));
  EIGX_HIP_CHECK(hipStreamCreateWithFlags(&g_ctx.side_stream, hipStreamNonBlocking));
  for (int q = 0; q < Context::kAux; ++q)
    EIGX_HIP_CHECK(hipStreamCreateWithFlags(&g_ctx.aux[q], hipStreamNonBlocking));
  for (int q = 0; q <= Context::kAux; ++q)
    EIGX_HIP_CHECK(hipEventCreateWithFlags(&g_ctx.aux_ev[q], hipEventDisableTiming));
  EIGX_HIP_CHECK(hipEventCreateWithFlags(&g_ctx.bt_ev, hipEventDisableTiming));
  EIGX_HIP_CHECK(hipEventCreateWithFlags(&g_ctx.dc_ev, hipEventDisableTiming));
  {
    // highest priority: its own hardware queue (the plain streams share four), and the small latency-bound kernels of the
    // next D&C pass get CU slots while the current pass's product fills the chip
    int prio_lo = 0, prio_hi = 0;
    EIGX_HIP_CHECK(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
    EIGX_HIP_CHECK(hipStreamCreateWithPriority(&g_ctx.dc_stream, hipStreamNonBlocking, prio_hi));
  }
  EIGX_HIP_CHECK(hipEventCreateWithFlags(&g_ctx.dc_b_ev, hipEventDisableTiming));
  EIGX_HIP_CHECK(hipEventCreateWithFlags(&g_ctx.dc_z_ev, hipEventDisableTiming));
  g_ctx.bt_stream = g_ctx.side_stream;
  g_ctx.initialized = true;
  g_ctx.errinfo = 0;
  return EIGX_OK;
}

int eigx_free(void) {
  if (!g_ctx.initialized) return EIGX_OK;
  EIGX_HIP_CHECK(hipSetDevice(g_ctx.device));
  EIGX_HIP_CHECK(hipDeviceSynchronize());
  if (g_ctx.grid.nranks > 1) comm_free(g_ctx);
  g_ctx.pool.release();
  for (hipEvent_t e : g_ctx.prof_ev) EIGX_HIP_CHECK(hipEventDestroy(e));
  EIGX_HIP_CHECK(hipStreamDestroy(g_ctx.stream));
  EIGX_HIP_CHECK(hipStreamDestroy(g_ctx.side_stream));
  for (int q = 0; q < Context::kAux; ++q) EIGX_HIP_CHECK(hipStreamDestroy(g_ctx.aux[q]));
  for (int q = 0; q <= Context::kAux; ++q) EIGX_HIP_CHECK(hipEventDestroy(g_ctx.aux_ev[q]));
  EIGX_HIP_CHECK(hipEventDestroy(g_ctx.bt_ev));
  EIGX_HIP_CHECK(hipEventDestroy(g_ctx.dc_ev));
  EIGX_HIP_CHECK(hipStreamDestroy(g_ctx.dc_stream));
  g_ctx.bt_stream = nullptr;
  EIGX_HIP_CHECK(hipEventDestroy(g_ctx.dc_b_ev));
  EIGX_HIP_CHECK(hipEventDestroy(g_ctx.dc_z_ev));
  g_ctx = Context();
  return EIGX_OK;
}

int eigx_get_version(int* version, char* date32, char* vcode32) {
  if (version) *version = 10;  // 0.10 of this library (tracks the reference's 2.13 API)
  if (date32) { memset(date32, 0, 32); strncpy(date32, "2026-10", 31); }
  if (vcode32) { memset(vcode32, 0, 32); strncpy(vcode32, "eigenexa_amd gfx950", 31); }
  return EIGX_OK;
}

int eigx_get_procs(int* procs, int* x_procs, int* y_procs) {
  if (!g_ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  if (procs) *procs = g_ctx.grid.nranks;
  if (x_procs) *x_procs = g_ctx.grid.Px;
  if (y_procs) *y_procs = g_ctx.grid.Py;
  return EIGX_OK;
}

int eigx_get_id(int* id, int* x_id, int* y_id) {
  if (!g_ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  if (id) *id = g_ctx.grid.rank + 1;
  if (x_id) *x_id = g_ctx.grid.px + 1;
  if (y_id) *y_id = g_ctx.grid.py + 1;
  return EIGX_OK;
}

int eigx_get_comm(int* x_color, int* x_key, int* y_color, int* y_key) {
  if (!g_ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  const Grid& g = g_ctx.grid;
  if (x_color) *x_color = g.py + 1;
  if (x_key) *x_key = g.px + 1;
  if (y_color) *y_color = g.px + 1;
  if (y_key) *y_key = g.py + 1;
  return EIGX_OK;
}

double eigx_comm_seconds(void) { return g_ctx.timers[4]; }

int eigx_comm_info(char* buf, int len) {
  if (!g_ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  return comm_info(g_ctx, buf, len);
}

int eigx_get_errinfo(int64_t* info) {
  if (info) *info = g_ctx.errinfo;
  return EIGX_OK;
}

// ---- index helpers: formulas of src/eigen_libs0.F:1825 (loop_start), :1911 (loop_end),
// :1995 (l2g), :2079 (g2l), :2163 (owner_node), :2247 (owner_index); all 1-based. --------------
int eigx_loop_start(int istart, int nnod, int inod) { return (istart + nnod - 1 - inod) / nnod + 1; }
int eigx_loop_end(int iend, int nnod, int inod) { return (iend + nnod - inod) / nnod; }
int eigx_translate_l2g(int ictr, int nnod, int inod) { return (ictr - 1) * nnod + inod; }
int eigx_translate_g2l(int ictr, int nnod, int inod) { (void)inod; return (ictr - 1) / nnod + 1; }
int eigx_owner_node(int ictr, int nnod, int inod) { (void)inod; return (ictr - 1) % nnod + 1; }
int eigx_owner_index(int ictr, int nnod, int inod) {
  return ((ictr - 1) % nnod + 1 == inod) ? (ictr - 1) / nnod + 1 : -1;
}

int eigx_matdims_for_grid(int n, int x_procs, int y_procs, int m_forward, int m_backward, char mode, int* nx, int* ny) {
  if (!nx || !ny || x_procs < 1 || y_procs < 1) return EIGX_ERR_BAD_ARG;
  (void)m_forward;
  if (n <= 0) { *nx = -1; *ny = -1; return EIGX_ERR_BAD_ARG; }
  const int Px = x_procs, Py = y_procs;
  const int mb = m_backward > 0 ? m_backward : 128;
  const int n1 = ceil_div(n, Px);
  const int n2 = ceil_div(n, Py);
  int lnx;
  int64_t lny;
  if (mode == 'M' || mode == 'm') {            // minimal extents (src/eigen_libs0.F:1283-1287)
    lnx = n1; lny = n2;
  } else if (mode == 'L' || mode == 'l') {     // nx rounded to 32 (src/eigen_libs0.F:1288-1293)
    lnx = ceil_div(n1, 32) * 32; lny = n2;
  } else {
    lnx = ceil_div(n1, 64) * 64 + 32;  // odd multiple of 32, >= CSTAB's choice + slack
    if (lnx < n1 + 64) lnx += 64;
    const int NB = mb > 64 ? mb : 64;
    // nmz / nmw of src/eigen_libs0.F:1318-1330: the larger of "local extent rounded to NB, plus one" and "blocks of NB
    // dealt to the processes"
    int64_t nmz = (int64_t)ceil_div(n1, NB) * NB + 1;
    const int64_t nmz2 = (int64_t)ceil_div(ceil_div(n, NB), Px) * NB;
    if (nmz2 > nmz) nmz = nmz2;
    int64_t nmw = (int64_t)ceil_div(n2, NB) * NB + 1;
    const int64_t nmw2 = (int64_t)ceil_div(ceil_div(n, NB), Py) * NB;
    if (nmw2 > nmw) nmw = nmw2;
    nmz += NB; nmw += NB;                // slack of one more block (the reference's z doubles as D&C workspace)
    const int64_t big = nmz > lnx ? nmz : lnx;
    lny = ceil_div64(big * nmw, lnx);
    if (lny < n2) lny = n2;
    lnx = hbm_ld(lnx);                 // the solvers work in place on a(nx, *): column shift of 4 - 12 KiB (eigx_common.h)
  }
  // the default build of the reference takes the maximum with FS_get_matdims (src/eigen_libs.F:139-146,
  // src/FS_libs.F90:356-375), for every mode
  {
    const int P = Px * Py;
    const int nf = ceil_div(n, P);
    const int64_t nx0 = (int64_t)nf * (P / Px), ny0 = (int64_t)nf * (P / Py);
    if (nx0 > lnx) lnx = (int)nx0;
    if (ny0 > lny) lny = ny0;
  }
  // 32-bit index guard of src/eigen_libs0.F:1349-1365
  const int pmin = Px < Py ? Px : Py;
  const int64_t side = ceil_div64(ceil_div(n, pmin), 64) * 64;
  if ((side * side >= ((int64_t)1 << 31) || lny >= ((int64_t)1 << 31)) && !(getenv("EIGX_ALLOW_64BIT"))) {
    *nx = -1; *ny = -1;
    return EIGX_ERR_TOO_LARGE;
  }
  *nx = lnx;
  *ny = (int)lny;
  return EIGX_OK;
}

// ---- matdims ------------------------------------------------------------------------------------
// The reference picks nx by a cache-set heuristic (CSTAB_get_optdim, src/CSTAB.F:73-131: an odd
// multiple of 32 nudged off A64FX cache aliasing) and ny so that z can double as D&C workspace
// (src/eigen_libs0.F:1297-1343).  The contract that matters to callers is "allocate a(nx,ny),
// z(nx,ny)"; we return extents >= the reference's (tests/test_host.py sweeps sizes and grids against a restatement
// of the reference's formulas): nx = ceil(n/Px) rounded up to an odd multiple of 32 plus one more 64 step of
// slack -- and, where the reference nudges nx off A64FX cache aliasing, off the MI355X memory-channel aliasing instead
// (hbm_ld, eigx_common.h) -- ny from the same nmz/nmw formula.
int eigx_get_matdims(int n, int* nx, int* ny, int m_forward, int m_backward, char mode) {
  if (!g_ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  return eigx_matdims_for_grid(n, g_ctx.grid.Px, g_ctx.grid.Py, m_forward, m_backward, mode, nx, ny);
}

int64_t eigx_memory_internal(int n, int lda, int ldz, int m_forward, int m_backward) {
  if (!g_ctx.initialized) return -1;
  return solver_workspace_bytes(g_ctx, n, lda, ldz, m_forward, m_backward);
}

int64_t eigx_held_bytes(void) {
  if (!g_ctx.initialized) return -1;
  int64_t t = 0;
  for (const auto& kv : g_ctx.pool.bufs) t += (int64_t)kv.second.bytes;
  return t + comm_held_bytes(g_ctx);
}

int64_t eigx_held_bytes_named(const char* prefix) {
  if (!g_ctx.initialized || !prefix) return -1;
  const std::string pre(prefix);
  int64_t t = 0;
  for (const auto& kv : g_ctx.pool.bufs)
    if (kv.first.compare(0, pre.size(), pre) == 0) t += (int64_t)kv.second.bytes;
  return t;
}

int eigx_get_timers(double* out16) {
  if (!out16) return EIGX_ERR_BAD_ARG;
  for (int i = 0; i < 16; ++i) out16[i] = g_ctx.timers[i];
  return EIGX_OK;
}

int eigx_profile(int stride) {
  if (!g_ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  g_ctx.prof_stride = stride > 0 ? stride : 0;
  g_ctx.prof_used = 0;
  g_ctx.prof_kind.clear();
  g_ctx.prof_units.clear();
  return EIGX_OK;
}

int eigx_profile_read(double* out6) {
  if (!g_ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  if (!out6) return EIGX_ERR_BAD_ARG;
  EIGX_HIP_CHECK(hipSetDevice(g_ctx.device));
  EIGX_HIP_CHECK(hipStreamSynchronize(g_ctx.stream));
  for (int q = 0; q < 6; ++q) out6[q] = 0.0;
  for (size_t q = 0; q < g_ctx.prof_kind.size(); ++q) {
    float ms = 0.f;
    EIGX_HIP_CHECK(hipEventElapsedTime(&ms, g_ctx.prof_ev[2 * q], g_ctx.prof_ev[2 * q + 1]));
    if (g_ctx.prof_kind[q] > 1) continue;   // kinds 2.. are the multi-rank step breakdown (eigx_profile_read_kinds)
    const int k = g_ctx.prof_kind[q] ? 3 : 0;
    out6[k + 0] += 1.0;
    out6[k + 1] += g_ctx.prof_units[q];
    out6[k + 2] += 1e-3 * ms;
  }
  return EIGX_OK;
}

int eigx_profile_read_kinds(double* out, int nkinds) {
  if (!g_ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  if (!out || nkinds < 1) return EIGX_ERR_BAD_ARG;
  EIGX_HIP_CHECK(hipSetDevice(g_ctx.device));
  EIGX_HIP_CHECK(hipStreamSynchronize(g_ctx.stream));
  for (int q = 0; q < 3 * nkinds; ++q) out[q] = 0.0;
  for (size_t q = 0; q < g_ctx.prof_kind.size(); ++q) {
    const int k = g_ctx.prof_kind[q];
    if (k < 0 || k >= nkinds) continue;
    float ms = 0.f;
    EIGX_HIP_CHECK(hipEventElapsedTime(&ms, g_ctx.prof_ev[2 * q], g_ctx.prof_ev[2 * q + 1]));
    out[3 * k + 0] += 1.0;
    out[3 * k + 1] += g_ctx.prof_units[q];
    out[3 * k + 2] += 1e-3 * ms;
  }
  return EIGX_OK;
}

int eigx_device_synchronize(void) {
  if (!g_ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  EIGX_HIP_CHECK(hipSetDevice(g_ctx.device));
  EIGX_HIP_CHECK(hipDeviceSynchronize());
  return EIGX_OK;
}

void* eigx_malloc_dev(int64_t bytes) {
  if (!g_ctx.initialized) return nullptr;
  void* p = nullptr;
  if (hipMalloc(&p, (size_t)bytes) != hipSuccess) return nullptr;
  return p;
}
int eigx_free_dev(void* p) {
  if (p) EIGX_HIP_CHECK(hipFree(p));
  return EIGX_OK;
}
int eigx_memcpy_h2d(void* dst, const void* src, int64_t bytes) {
  EIGX_HIP_CHECK(hipMemcpy(dst, src, (size_t)bytes, hipMemcpyHostToDevice));
  return EIGX_OK;
}
int eigx_memcpy_d2h(void* dst, const void* src, int64_t bytes) {
  EIGX_HIP_CHECK(hipMemcpy(dst, src, (size_t)bytes, hipMemcpyDeviceToHost));
  return EIGX_OK;
}

int eigx_tune(int key, int value) {
  if (key == 0) return set_gemm_variant(value);
  if (key == 1) return set_bisect_threads(value);
  if (key == 2) return set_bt_q(value);
  if (key == 3 || key == 4 || key == 5 || key == 10 || key == 11) return set_reduce_knob(key, value);
  if (key == 12) return (value >= 0 && value <= 2) ? set_reduce_knob(key, value) : -1;
  if (key == 6) return set_gemm_cstream(value);
  if (key == 7) return value > 0 ? set_reduce_knob(key, value) : -1;
  if (key == 8) return set_dc_chunk(value);
  if (key == 9) return comm_set_bounce(value);
  if (key == 15) return set_dc_pipe(value);    // D&C on one GPU: next pass's deflation / secular equations under this pass's product
  if (key == 16) return set_dc_batch(value);   // D&C on one GPU: one product launch per low height
  if (key == 17 || key == 18 || key == 19) return set_range_knob(key, value);   // index-range solves (subset.hip)
  if (key == 20) return set_tri_nb(value);     // outer block width of the triangular stages (tri.hip)
  if (key == 21) return set_batch_nmax(value); // largest n served by the batch kernel of eigx_s_batch (batch.hip)
  if (key == 22) return set_hbatch_nmax(value);   // the same for eigx_h_batch (hbatch.hip)
  if (key == 23) return set_gbatch_nmax(value);   // the same for eigx_gev_batch (gbatch.hip)
  if (key == 24) return set_hgbatch_nmax(value);  // the same for eigx_hgev_batch (hgbatch.hip)
  if (key == 25) return set_gemm_latec_kmax(value);  // largest K of the one-GPU trailing update's late-C path, 0 = never (gemm_f64.hip)
  if (key == 26) return set_batch_range_route(value);   // eigx_s_batch_range, eigx_h_batch_range, eigx_gev_batch_range, eigx_hgev_batch_range: 0 automatic, 1 window kernel where eligible, 2 full solve + slice
  if (key == 27) return set_batch_range_accept(value);  // its acceptance bound in percent, 0 .. 101 (101 refuses every matrix) (batch_range.hip)
  return -1;
}

int eigx_dgemm_dev(char opa, char opb, int m, int n, int k, double alpha, const double* a, int lda,
                   const double* b, int ldb, double beta, double* c, int ldc, int tri_upper) {
  if (!g_ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  EIGX_HIP_CHECK(hipStreamSynchronize(nullptr));   // the caller's default-stream work on the operands
  dgemm_dev(g_ctx.stream, opa, opb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc, tri_upper ? 1 : 0,
            &g_ctx.grid);
  EIGX_HIP_CHECK(hipStreamSynchronize(g_ctx.stream));
  return EIGX_OK;
}

int eigx_dgemm_gather_dev(char opa, char opb, int m, int n, int k, double alpha, const double* a, int lda,
                          const double* b, int ldb, double beta, double* c, int ldc, const int* kmap_a,
                          const int* kmap_b) {
  if (!g_ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  EIGX_HIP_CHECK(hipStreamSynchronize(nullptr));
  dgemm_dev(g_ctx.stream, opa, opb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc, 0, nullptr, kmap_a, nullptr, 1, 0,
            0, 0, 1, 0, 0, 0, 1, 0, kmap_b);
  EIGX_HIP_CHECK(hipStreamSynchronize(g_ctx.stream));
  return EIGX_OK;
}

}  // extern "C"
