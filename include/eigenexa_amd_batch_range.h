/* eigenexa_amd_batch_range.h -- the windowed batched small eigensolves of libeigenexa_amd.so (an EXTENSION, not in the
 * reference).  Part of the C-ABI of eigenexa_amd.h, which includes this file: include that header.  The entries have a file of
 * their own because the list of entries of eigenexa_amd.h and the ctypes table that mirrors it (eigenexa_amd/_lib.py,
 * SIGNATURES) are held fixed, name by name and in order, by tests/test_api_frontend.py; these are mirrored by
 * _lib.BATCH_RANGE_SIGNATURES and held against it by tests/test_batch_range.py in the same way. */
#ifndef EIGENEXA_AMD_BATCH_RANGE_H
#define EIGENEXA_AMD_BATCH_RANGE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Windowed batched eigensolves -- EXTENSION, not in the reference: eigenpairs il .. iu (1-based, inclusive, of the ascending
 * spectrum; the same window for every matrix) of `batch` real symmetric matrices of one size n.  One GPU only: with more than
 * one rank the entries print the line of the range entries and return EIGX_ERR_BAD_ARG.
 * Storage of a as for eigx_s_batch: matrix k (0-based) is a + k stride_a (leading dimension lda), upper triangle significant
 * (the strict lower triangle, the rows beyond n and the gaps may hold anything, NaN included), destroyed.  With
 * m = iu - il + 1: w(1:m, k) at w + k ldw receives eigenvalues il .. iu of matrix k, ascending; z(1:n, 1:m, k) at z + k stride_z
 * (leading dimension ldz) the orthonormal eigenvectors.  Nothing else of w and z is written.
 * mode 'A' eigenpairs, 'N' eigenvalues only (z may be NULL; ldz and stride_z are ignored); anything else is EIGX_ERR_BAD_ARG.
 * EIGX_ERR_BAD_ARG also unless n >= 1, batch >= 0, 1 <= il <= iu <= n, lda >= n, ldw >= m, stride_a >= lda n where batch > 1,
 * a and w non-NULL, and in mode 'A' z non-NULL, ldz >= n, stride_z >= ldz m where batch > 1; nothing is touched then.
 * batch = 0 returns EIGX_OK and touches nothing.
 * Per-matrix status: info[k] = 0, EIGX_ERR_NONFINITE (a NaN / Inf in the upper triangle: w(1:m, k) = NaN, z(:, :, k)
 * untouched) or EIGX_ERR_INTERNAL (the QL iteration of the full solve used up its budget: w(1:m, k) = NaN, z(:, :, k)
 * untouched).  info may be NULL; in the _dev form it is a device int array.  A failed matrix never disturbs the others; the
 * call returns EIGX_OK or the code of the failed matrix with the lowest index, and eigx_get_errinfo gives -1 then.
 * Method (csrc/batch_range.hip), three routes:
 *   1  the window kernel: one launch, one workgroup per matrix, everything in LDS: the tridiagonalisation of eigx_s_batch
 *      without the accumulation of Q, Sturm-count multi-section for the m eigenvalues (no QL sweep), and in mode 'A' inverse
 *      iteration (one lane per vector), two Gram-Schmidt passes over the window, Rayleigh-Ritz on the m x m projection and the
 *      reflectors applied to m columns.  It serves mode 'N' for any m and mode 'A' for m <= 16 (n <= 96) or m <= 4
 *      (97 <= n <= 128).  A matrix whose vectors lose more than the bound of eigx_tune key 27 in the second Gram-Schmidt pass is
 *      not finished by it but solved again by route 2 (the redo); whether that happens depends on the matrix alone.
 *   2  the batch kernel of eigx_s_batch into workspace (pool buffers "batch.r*", at most 256 MiB at a time) and a gather of the
 *      window: w and z are bit for bit the slices of what eigx_s_batch_dev returns.
 *   3  n above the cutoff of eigx_s_batch (eigx_tune key 21): eigx_s_range_dev(n, il, iu, ..., m_forward = 48, m_backward = 128,
 *      mode) matrix by matrix, bit for bit what the caller's own loop gives.
 * Which of routes 1 and 2 a call takes: eigx_tune key 26 (default: by the measured table of DESIGN section 8n).  On either the
 * arithmetic of a matrix depends on n and the window alone: the result at position k of a batch is bit for bit that of the
 * matrix solved alone, and two runs agree bit for bit.  The device form waits on the default stream on entry and returns after
 * the result is complete.  eigx_get_timers [0] = the seconds of the call, the rest 0.  The host form stages a, w and z through
 * pool buffers "brange.h*"; w comes back for every matrix, z for those that succeeded. */
int eigx_s_batch_range(int n, int batch, int il, int iu, double* a, int lda, int64_t stride_a, double* w, int ldw, double* z, int ldz,
                       int64_t stride_z, char mode, int* info);
int eigx_s_batch_range_dev(int n, int batch, int il, int iu, double* a_dev, int lda, int64_t stride_a, double* w_dev, int ldw,
                           double* z_dev, int ldz, int64_t stride_z, char mode, int* info_dev);
/* What the last call of a windowed batched entry did -- the two above, their Hermitian siblings eigx_h_batch_range[_dev]
 * (eigenexa_amd_hbatch_range.h) or their pencil siblings eigx_gev_batch_range[_dev] (eigenexa_amd_gbatch_range.h) and
 * eigx_hgev_batch_range[_dev] (eigenexa_amd_hgbatch_range.h), whichever ran last: *route = 1, 2 or 3 as listed (1 also when some matrices went to the redo),
 * *m = iu - il + 1, *redone = the number of matrices the acceptance test of route 1 sent to route 2.  Any pointer may be NULL.
 * Returns EIGX_OK. */
int eigx_batch_range_info(int* route, int* m, int* redone);

#ifdef __cplusplus
}
#endif
#endif /* EIGENEXA_AMD_BATCH_RANGE_H */
