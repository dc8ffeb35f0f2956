/* eigenexa_amd_hbatch_range.h -- the windowed batched small complex Hermitian eigensolves of libeigenexa_amd.so (an EXTENSION, not
 * in the reference).  Part of the C-ABI of eigenexa_amd.h, which includes this file: include that header.  The entries have a file
 * of their own because the lists of entries of eigenexa_amd.h and eigenexa_amd_batch_range.h and the ctypes tables that mirror
 * them are held fixed, name by name, by tests/test_api_frontend.py and tests/test_batch_range.py; these are mirrored by
 * _lib.HBATCH_RANGE_SIGNATURES and held against it by tests/test_hbatch_range.py in the same way. */
#ifndef EIGENEXA_AMD_HBATCH_RANGE_H
#define EIGENEXA_AMD_HBATCH_RANGE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Windowed batched Hermitian eigensolves -- EXTENSION, not in the reference: eigenpairs il .. iu (1-based, inclusive, of the
 * ascending spectrum; the same window for every matrix) of `batch` complex Hermitian matrices of one size n.  The contract is
 * that of eigx_s_batch_range (eigenexa_amd_batch_range.h) with the storage of eigx_h_batch.  One GPU only: with more than one
 * rank the entries print the line of the range entries and return EIGX_ERR_BAD_ARG.
 * a and z are interleaved complex (re, im pairs of doubles); lda, ldz, stride_a and stride_z count complex elements.  Matrix k
 * (0-based) is a + 2 k stride_a doubles (leading dimension lda), upper triangle significant, of the diagonal only the real parts
 * are read (the strict lower triangle, the imaginary parts of the diagonal, the rows beyond n and the gaps may hold anything, NaN
 * included), destroyed.  With m = iu - il + 1: w(1:m, k) at w + k ldw receives eigenvalues il .. iu of matrix k, real and
 * ascending; z(1:n, 1:m, k) at z + 2 k stride_z doubles (leading dimension ldz) the complex orthonormal eigenvectors.  Nothing
 * else of w and z is written.
 * mode 'A' eigenpairs, 'N' eigenvalues only (z may be NULL; ldz and stride_z are ignored); anything else is EIGX_ERR_BAD_ARG.
 * EIGX_ERR_BAD_ARG also unless n >= 1, batch >= 0, 1 <= il <= iu <= n, lda >= n, ldw >= m, stride_a >= lda n where batch > 1,
 * a and w non-NULL, and in mode 'A' z non-NULL, ldz >= n, stride_z >= ldz m where batch > 1; nothing is touched then.
 * batch = 0 returns EIGX_OK and touches nothing.
 * Per-matrix status: info[k] = 0, EIGX_ERR_NONFINITE (a NaN / Inf in what is read of the upper triangle: w(1:m, k) = NaN,
 * z(:, :, k) untouched) or EIGX_ERR_INTERNAL (the QL iteration of the full solve used up its budget: w(1:m, k) = NaN, z(:, :, k)
 * untouched).  info may be NULL; in the _dev form it is a device int array.  A failed matrix never disturbs the others; the
 * call returns EIGX_OK or the code of the failed matrix with the lowest index, and eigx_get_errinfo gives -1 then.
 * Method (csrc/hbatch_range.hip), three routes:
 *   1  the window kernel: one launch, one workgroup per matrix, everything in LDS: the Hermitian tridiagonalisation and the
 *      phase chain of eigx_h_batch without the accumulation of Q, then on the real tridiagonal matrix the window stage of
 *      eigx_s_batch_range (Sturm-count multi-section, and in mode 'A' inverse iteration, two Gram-Schmidt passes, Rayleigh-Ritz
 *      on the m x m projection), the phases and the reflectors applied to m complex columns.  It serves mode 'N' for any m and
 *      n <= 96, and mode 'A' for m <= 16 and n <= 64.  A matrix whose vectors lose more than the bound of eigx_tune key 27 in the
 *      second Gram-Schmidt pass is not finished by it but solved again by route 2 (the redo); whether that happens depends on
 *      the matrix alone.
 *   2  the batch kernel of eigx_h_batch into workspace (pool buffers "hbatch.r*", at most 256 MiB at a time) and a gather of the
 *      window: w and z are bit for bit the slices of what eigx_h_batch_dev returns.  Mode 'A' at 65 <= n <= 96 always takes it.
 *   3  n above the cutoff of eigx_h_batch (eigx_tune key 22): eigx_h_range_dev(n, il, iu, ..., m_forward = 48, m_backward = 128,
 *      mode) matrix by matrix, bit for bit what the caller's own loop gives.
 * Which of routes 1 and 2 a call takes: eigx_tune key 26 (default: by the measured table of DESIGN section 8o; a cell that is
 * not measured takes route 2).  On either the arithmetic of a matrix depends on n and the window alone: the result at position k
 * of a batch is bit for bit that of the matrix solved alone, and two runs agree bit for bit.  The device form waits on the
 * default stream on entry and returns after the result is complete.  eigx_get_timers [0] = the seconds of the call, the rest 0.
 * The host form stages a, w and z through pool buffers "hbrange.h*"; w comes back for every matrix, z for those that succeeded.
 * eigx_batch_range_info (eigenexa_amd_batch_range.h) reports the last call of these entries as well. */
int eigx_h_batch_range(int n, int batch, int il, int iu, double* a, int lda, int64_t stride_a, double* w, int ldw, double* z, int ldz,
                       int64_t stride_z, char mode, int* info);
int eigx_h_batch_range_dev(int n, int batch, int il, int iu, double* a_dev, int lda, int64_t stride_a, double* w_dev, int ldw,
                           double* z_dev, int ldz, int64_t stride_z, char mode, int* info_dev);

#ifdef __cplusplus
}
#endif
#endif /* EIGENEXA_AMD_HBATCH_RANGE_H */
