// gemm_lab.hip -- test interface to the GEMM dispatcher (include/eigenexa_amd_gemm_lab.h): every argument of dgemm_dev that
// has a caller, and the table launch, for tests/test_gemm_paths.py.  Nothing in the library calls these entries.
#include "eigx_context.h"
#include "../../include/eigenexa_amd.h"
#include "../../include/eigenexa_amd_gemm_lab.h"
#include <climits>

using namespace eigx;

extern "C" {

int eigx_dgemm_ex_dev(char opa, char opb, int m, int n, int k, double alpha, const double* a, int lda, const double* b,
                      int ldb, double beta, double* c, int ldc, int tri_mode, int px_n, int px, int py_n, int py, int batch,
                      int64_t stride_a, int64_t stride_b, int64_t stride_c, int batch2, int64_t stride_a2, int64_t stride_b2,
                      int64_t stride_c2, int tn_lo, int tn_hi, const int* kmap_a, const int* kmap_b) {
  if (!g_ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  if (tri_mode < 0 || tri_mode > 2) return EIGX_ERR_BAD_ARG;
  if (px_n < 1 || py_n < 1 || px < 0 || px >= px_n || py < 0 || py >= py_n) return EIGX_ERR_BAD_ARG;
  if (kmap_a || kmap_b) {   // what dgemm_dev aborts on
    const bool nt = (opa == 'N' || opa == 'n') && (opb == 'T' || opb == 't');
    if (!nt || !kmap_a || !kmap_b) return EIGX_ERR_BAD_ARG;
  }
  Grid grid;
  grid.Px = px_n; grid.px = px; grid.Py = py_n; grid.py = py;
  grid.nranks = px_n * py_n;
  EIGX_HIP_CHECK(hipStreamSynchronize(nullptr));   // the caller's default-stream work on the operands
  dgemm_dev(g_ctx.stream, opa, opb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc, tri_mode, &grid, kmap_a, nullptr, batch,
            (long)stride_a, (long)stride_b, (long)stride_c, batch2, (long)stride_a2, (long)stride_b2, (long)stride_c2, 1, 0,
            kmap_b, tn_lo, tn_hi);
  EIGX_HIP_CHECK(hipStreamSynchronize(g_ctx.stream));
  return EIGX_OK;
}

int eigx_dgemm_tri2_launch_tiles(int m, int n, int px_n, int px, int py_n, int py, int tn_lo, int tn_hi) {
  if (px_n < 1 || py_n < 1 || px < 0 || px >= px_n || py < 0 || py >= py_n) return EIGX_ERR_BAD_ARG;
  Grid grid;
  grid.Px = px_n; grid.px = px; grid.Py = py_n; grid.py = py;
  return gemm_tri2_launch_tiles(m, n, grid, tn_lo, tn_hi);
}

int eigx_dgemm_gather_table_dev(int nbatch, const int64_t* entries, const double* a, int lda, const double* b, int ldb,
                                double* c, int ldc, const int* kmap_a, const int* kmap_b) {
  if (!g_ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  if (nbatch < 0 || (nbatch > 0 && (!entries || !kmap_a || !kmap_b))) return EIGX_ERR_BAD_ARG;
  if (nbatch == 0) return EIGX_OK;
  std::vector<GemmBatch> tab(nbatch);
  int maxM = 0, maxN = 0;
  for (int i = 0; i < nbatch; ++i) {
    const int64_t* e = entries + (size_t)8 * i;
    if (e[0] < 0 || e[1] < 0 || e[2] < 0 || e[0] > INT_MAX || e[1] > INT_MAX || e[2] > INT_MAX) return EIGX_ERR_BAD_ARG;
    if (e[6] < INT_MIN || e[6] > INT_MAX || e[7] < INT_MIN || e[7] > INT_MAX) return EIGX_ERR_BAD_ARG;
    GemmBatch& t = tab[i];
    t.M = (int)e[0]; t.N = (int)e[1]; t.K = (int)e[2]; t.pad = 0;
    t.offA = (long)e[3]; t.offB = (long)e[4]; t.offC = (long)e[5];
    t.offKA = (int)e[6]; t.offKB = (int)e[7];
    if (t.M > maxM) maxM = t.M;
    if (t.N > maxN) maxN = t.N;
  }
  GemmBatch* tab_dev = nullptr;
  if (hipMalloc(&tab_dev, (size_t)nbatch * sizeof(GemmBatch)) != hipSuccess) { (void)hipGetLastError(); return EIGX_ERR_NO_MEMORY; }
  EIGX_HIP_CHECK(hipStreamSynchronize(nullptr));
  EIGX_HIP_CHECK(hipMemcpyAsync(tab_dev, tab.data(), (size_t)nbatch * sizeof(GemmBatch), hipMemcpyHostToDevice, g_ctx.stream));
  dgemm_gather_batch_dev(g_ctx.stream, tab_dev, nbatch, maxM, maxN, a, lda, b, ldb, c, ldc, kmap_a, kmap_b);
  EIGX_HIP_CHECK(hipStreamSynchronize(g_ctx.stream));   // the table is read until the launch has drained
  EIGX_HIP_CHECK(hipFree(tab_dev));
  return EIGX_OK;
}

}  // extern "C"
