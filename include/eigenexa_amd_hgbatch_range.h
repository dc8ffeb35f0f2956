/* eigenexa_amd_hgbatch_range.h -- the windowed batched small complex generalised eigensolves of libeigenexa_amd.so (an EXTENSION, not
 * in the reference).  Part of the C-ABI of eigenexa_amd.h, which includes this file: include that header.  The entries have a file
 * of their own because the lists of entries of the other headers and the ctypes tables that mirror them are held fixed, name by
 * name, by tests/test_api_frontend.py, tests/test_hgbatch.py, tests/test_batch_range.py, tests/test_hbatch_range.py and
 * tests/test_gbatch_range.py; these are mirrored by _lib.HGBATCH_RANGE_SIGNATURES and held against it by
 * tests/test_hgbatch_range.py in the same way. */
#ifndef EIGENEXA_AMD_HGBATCH_RANGE_H
#define EIGENEXA_AMD_HGBATCH_RANGE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Windowed batched complex generalised eigensolves -- EXTENSION, not in the reference: eigenpairs il .. iu (1-based, inclusive, of
 * the ascending spectrum; the same window for every pencil) of `batch` Hermitian-definite pencils A x = lambda B x of one size n.
 * The contract is that of eigx_gev_batch_range (eigenexa_amd_gbatch_range.h) for il, iu, w and z with the storage of
 * eigx_hgev_batch (eigenexa_amd_hgbatch.h) for a, b and z.  One GPU only: with more than one rank the entries print the line of
 * the range entries and return EIGX_ERR_BAD_ARG.
 * a, b and z hold interleaved complex numbers (re, im); strides and leading dimensions count complex elements, ldw counts
 * doubles.  Pencil k (0-based) is a + 2 k stride_a (leading dimension lda) and b + 2 k stride_b (ldb); the upper triangles are
 * significant, of the diagonals the real parts only (the strict lower triangles, the imaginary parts of the diagonals, the rows
 * beyond n and the gaps may hold anything, NaN included); a is destroyed; a, b and z do not overlap.  With m = iu - il + 1: the
 * real w(1:m, k) at w + k ldw receives eigenvalues il .. iu of pencil k, ascending; z(1:n, 1:m, k) at z + 2 k stride_z (leading
 * dimension ldz) the eigenvectors, normalised so that z^H B z = I_m.  Nothing else of w and z is written.
 * What comes back in b: for n at or below the cutoff of eigx_hgev_batch (eigx_tune key 24), for a pencil with info[k] = 0, the
 * upper triangle of b(:, :, k) holds U with B = U^H U and a real positive diagonal (its imaginary parts stored as 0.0), bit for
 * bit the U that eigx_hgev_batch_dev returns for that pencil, on every route and in both modes (U belongs to the caller's B, not
 * to a scaled copy); the strict lower triangle, the rows beyond n and the gaps are never written.  A failed pencil returns its b
 * as it was passed, w(1:m, k) = NaN and z(:, :, k) untouched.  Above the cutoff b is what eigx_hgev_range_dev leaves in it (U on
 * success; see route 3).
 * mode 'A' eigenpairs, 'N' eigenvalues only (z may be NULL; ldz and stride_z are ignored; U is still returned); anything else is
 * EIGX_ERR_BAD_ARG.  EIGX_ERR_BAD_ARG also unless n >= 1, batch >= 0, 1 <= il <= iu <= n, lda >= n, ldb >= n, ldw >= m,
 * stride_a >= lda n and stride_b >= ldb n where batch > 1, a, b and w non-NULL, and in mode 'A' z non-NULL, ldz >= n,
 * stride_z >= ldz m where batch > 1; nothing is touched then.  batch = 0 returns EIGX_OK and touches nothing.
 * Per-pencil status: info[k] = 0; EIGX_ERR_NONFINITE (a NaN / Inf in the upper triangle of A or of B, both scanned before
 * anything is factored); EIGX_ERR_NOT_SPD (a Cholesky pivot that is not > 0 or not finite, the rule of eigx_zchol_dev, or a
 * non-finite entry in the formed C; the kernels print no message); or EIGX_ERR_INTERNAL (the QL iteration of the full solve used
 * up its budget).  info may be NULL; in the _dev form it is a device int array.  A failed pencil never disturbs the others; the
 * call returns EIGX_OK or the code of the failed pencil with the lowest index, and eigx_get_errinfo gives -1 then.
 * Method (csrc/hgbatch_range.hip), three routes:
 *   1  the window kernel: one launch, one workgroup per pencil, the four split planes of both matrices in LDS: the scaling,
 *      B = U^H U and C = U^-H A U^-1 of eigx_hgev_batch (the same arithmetic in the same order), the Hermitian tridiagonalisation
 *      of C and its phase chain without the accumulation of Q, the window stage of eigx_s_batch_range on the real tridiagonal
 *      matrix (Sturm-count multi-section, and in mode 'A' inverse iteration, two Gram-Schmidt passes, Rayleigh-Ritz on the m x m
 *      projection), the phases and the reflectors applied to m complex columns and Z = U^-1 V on them.  It serves mode 'N' for any
 *      m and n <= 64, and mode 'A' for m <= 16 at n <= 32 and for m <= 8 at 33 <= n <= 64 (beside the four planes of that class
 *      the LDS of a workgroup holds eight window columns).  A pencil whose vectors lose more than the bound of eigx_tune key 27
 *      in the second Gram-Schmidt pass is not finished by it (nothing of it is written, b included) but solved again by route 2
 *      (the redo); whether that happens depends on the pencil alone.
 *   2  eigx_hgev_batch_dev on the caller's a and b, so that U lands in b, with w and z in workspace (pool buffers "hgbrange.r*",
 *      at most 256 MiB at a time) and a gather of the window: w and z are bit for bit the slices of what eigx_hgev_batch_dev
 *      returns.  Mode 'A' with m > 16, or with m > 8 at n >= 33, always takes it.
 *   3  n above the cutoff of eigx_hgev_batch (eigx_tune key 24): eigx_hgev_range_dev(n, il, iu, ..., mode) pencil by pencil, bit
 *      for bit what the caller's own loop gives; that entry takes every leading dimension >= n, so nothing is staged.  Such a
 *      pencil inherits that entry's behaviour: B is not scaled, the not-positive-definite message is printed once per failed
 *      pencil, and what a failed pencil leaves in w and b is that entry's.
 * Which of routes 1 and 2 a call takes: eigx_tune key 26 (default: by the measured table of DESIGN section 8q; a cell that is
 * not measured takes route 2).  On either the arithmetic of a pencil depends on n, the window and the route alone: the result at
 * position k of a batch is bit for bit that of the pencil solved alone, and two runs agree bit for bit.  The device form waits on
 * the default stream on entry and returns after the result is complete.  eigx_get_timers [0] = the seconds of the call, the rest
 * 0.  The host form stages a, b, w and z through pool buffers "hgbrange.h*"; w comes back for every pencil, z and b (as U) for
 * those that succeeded.  eigx_batch_range_info (eigenexa_amd_batch_range.h) reports the last call of these entries as well. */
int eigx_hgev_batch_range(int n, int batch, int il, int iu, double* a, int lda, int64_t stride_a, double* b, int ldb,
                          int64_t stride_b, double* w, int ldw, double* z, int ldz, int64_t stride_z, char mode, int* info);
int eigx_hgev_batch_range_dev(int n, int batch, int il, int iu, double* a_dev, int lda, int64_t stride_a, double* b_dev, int ldb,
                              int64_t stride_b, double* w_dev, int ldw, double* z_dev, int ldz, int64_t stride_z, char mode,
                              int* info_dev);

#ifdef __cplusplus
}
#endif
#endif /* EIGENEXA_AMD_HGBATCH_RANGE_H */
