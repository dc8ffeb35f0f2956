/* eigenexa_amd_gemm_lab.h -- a TEST INTERFACE to the fp64 GEMM dispatcher of libeigenexa_amd.so (csrc/gemm_f64.hip).
 * It is not part of the public C-ABI: eigenexa_amd.h does not include this file, nothing in the library or in the Python
 * package calls these entries, and they may change with the dispatcher.  They exist so that tests/test_gemm_paths.py can reach
 * every argument of the internal dgemm_dev / dgemm_gather_batch_dev (csrc/eigx_common.h) that the solvers use and that
 * eigx_dgemm_dev / eigx_dgemm_gather_dev do not expose.  Mirrored by _lib.LAB_SIGNATURES (eigenexa_amd/_lib.py) and held against
 * it by tests/test_gemm_paths.py.  Defined in csrc/gemm_lab.hip.
 * Both entries follow the frame of eigx_dgemm_dev: EIGX_ERR_NOT_INITIALIZED before eigx_init, wait for the default stream, run
 * on the library's stream, wait for it.  All arrays are device pointers unless said otherwise; strides and offsets count
 * doubles (ints for the maps). */
#ifndef EIGENEXA_AMD_GEMM_LAB_H
#define EIGENEXA_AMD_GEMM_LAB_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* C = alpha op(A) op(B) + beta C with every argument of dgemm_dev that has a caller:
 *   tri_mode        0 full; 1 the tiles of 128 x 128 that touch the upper triangle (square tile grid); 2 the same test on the
 *                   local block of a 2-D cyclic distribution: tile (tm, tn) is updated iff
 *                   tm 128 px_n + px <= min(tn 128 + 127, n - 1) py_n + py and tn_lo <= tn < tn_hi
 *   px_n, px, py_n, py   the process grid (rows px_n with this rank at px, columns py_n at py), built into a local Grid; the
 *                   grid of eigx_init is neither read nor changed
 *   batch, stride_* / batch2, stride_*2   batch x batch2 products, operand (i, j) at base + i stride + j stride2
 *   tn_lo, tn_hi    window of tile columns (tri_mode 1 and 2)
 *   kmap_a, kmap_b  gather maps (k-index -> column of A / of B), or NULL
 * Returns EIGX_ERR_BAD_ARG, and launches nothing, for a tri_mode outside 0 .. 2, a grid position outside its grid, and for the
 * combination that dgemm_dev aborts on: a gather map without opa = 'N', opb = 'T' and both maps.  Like BLAS, alpha == 0 and
 * k == 0 read neither A nor B, and beta == 0 does not read C; a map that is passed is still read at index 0 then. */
int eigx_dgemm_ex_dev(char opa, char opb, int m, int n, int k, double alpha, const double* a_dev, int lda, const double* b_dev,
                      int ldb, double beta, double* c_dev, int ldc, int tri_mode, int px_n, int px, int py_n, int py, int batch,
                      int64_t stride_a, int64_t stride_b, int64_t stride_c, int batch2, int64_t stride_a2, int64_t stride_b2,
                      int64_t stride_c2, int tn_lo, int tn_hi, const int* kmap_a_dev, const int* kmap_b_dev);

/* The table launch dgemm_gather_batch_dev: nbatch products C_b = A(:, kmap_a_b) B(:, kmap_b_b)^T of their own sizes in one
 * launch.  entries is a HOST array of 8 nbatch values, (M, N, K, offA, offB, offC, offKA, offKB) per product: offsets from
 * a_dev, b_dev, c_dev and from the two maps.  The entry copies them into a device table, takes the largest M and N for the
 * launch, and frees the table after the stream has drained.  EIGX_ERR_BAD_ARG for nbatch < 0, a NULL array or map with nbatch > 0, a
 * negative size or a value that does not fit the table's int fields; nbatch = 0 returns EIGX_OK and touches nothing. */
int eigx_dgemm_gather_table_dev(int nbatch, const int64_t* entries, const double* a_dev, int lda, const double* b_dev, int ldb,
                                double* c_dev, int ldc, const int* kmap_a_dev, const int* kmap_b_dev);

/* Host arithmetic only (no GPU, no eigx_init): the number of workgroups that the ring kernel's tri_mode 2 launch has for a
 * local m x n block on this grid and window.  It launches row groups of 8 tile rows (m <= 32768), each from the first tile
 * column in the window at which the group's first tile row is on or above the global diagonal, so the count is the sum over
 * the groups of (tile rows of the group) x (tile columns of the window at which tile (8 q, tn) is updated by the rule above).
 * More would only cost launches that return at once; fewer would lose tiles.  EIGX_ERR_BAD_ARG for a grid position outside
 * its grid. */
int eigx_dgemm_tri2_launch_tiles(int m, int n, int px_n, int px, int py_n, int py, int tn_lo, int tn_hi);

#ifdef __cplusplus
}
#endif
#endif /* EIGENEXA_AMD_GEMM_LAB_H */
