/* eigenexa_amd_gbatch.h -- the batched small generalised eigensolves of libeigenexa_amd.so (an EXTENSION, not in the
 * reference).  Part of the C-ABI of eigenexa_amd.h, which includes this file: include that header.  The entries have a file of
 * their own because the list of entries of eigenexa_amd.h and the ctypes table that mirrors it (eigenexa_amd/_lib.py,
 * SIGNATURES) are held fixed, name by name and in order, by tests/test_api_frontend.py; these are mirrored by
 * _lib.GBATCH_SIGNATURES and held against it by tests/test_gbatch.py in the same way. */
#ifndef EIGENEXA_AMD_GBATCH_H
#define EIGENEXA_AMD_GBATCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Batched small generalised eigensolves -- EXTENSION, not in the reference: `batch` symmetric-definite pencils A x = lambda B x
 * of one size n, each solved completely (LAPACK callers know the per-pencil operation as dsygv, itype 1).  One GPU only: with
 * more than one rank the two entries print the line of the range entries and return EIGX_ERR_BAD_ARG.
 * Storage as for eigx_s_batch, strides and leading dimensions in doubles: pencil k (0-based) is a + k stride_a (leading
 * dimension lda) and b + k stride_b (ldb); its eigenvalues come back in w + k ldw, ascending; its eigenvectors in z + k stride_z
 * (ldz), normalised so that z^T B z = I.  The upper triangles of a and b are significant (the strict lower triangles, the rows
 * beyond n and the gaps may hold anything, NaN included); a is destroyed (contents unspecified, no statistics); a, b and z do
 * not overlap.  Only w(1:n) and z(1:n, 1:n) of each pencil are written.  On exit, for a pencil with info[k] = 0, the upper
 * triangle of b(:, :, k) holds U with B = U^T U (the contract of eigx_gev_range; U belongs to the caller's B, not to a scaled
 * copy) and its strict lower triangle is unspecified; the rows of b beyond n and the gaps are never written; the b of a pencil
 * that failed with EIGX_ERR_NONFINITE is left as it was passed.
 * mode 'A' eigenpairs, 'N' eigenvalues only (z may be NULL; ldz and stride_z are ignored; U is still returned); anything else is
 * EIGX_ERR_BAD_ARG.  EIGX_ERR_BAD_ARG also unless n >= 1, batch >= 0, lda >= n, ldb >= n, ldw >= n, stride_a >= lda n and
 * stride_b >= ldb n where batch > 1, b non-NULL, and in mode 'A' ldz >= n, stride_z >= ldz n where batch > 1.  batch = 0 returns
 * EIGX_OK and touches nothing.
 * Per-pencil status: info[k] = 0; EIGX_ERR_NONFINITE (a NaN / Inf in the upper triangle of A or of B, both scanned before
 * anything is factored: w(:, k) = NaN, z(:, :, k) untouched); EIGX_ERR_NOT_SPD (a Cholesky pivot that is not > 0 or not finite,
 * the rule of eigx_chol_dev, or a non-finite entry in the formed C: w(:, k) = NaN, z(:, :, k) untouched; the batch kernel prints
 * no message); or EIGX_ERR_INTERNAL (the QL iteration used up its 30 n iterations: w(:, k) = NaN, z(:, :, k) unspecified).  info
 * may be NULL; in the _dev form it is a device int array.  A failed pencil never disturbs the others; the call returns EIGX_OK
 * or the code of the failed pencil with the lowest index.
 * Method (csrc/gbatch.hip): for n <= EIGX_GBATCH_NMAX one launch, one workgroup per pencil, both matrices in
 * LDS from load to store: B = U^T U, C = U^-T A U^-1 by two triangular substitutions, the reduction and QL iteration of
 * eigx_s_batch (the same code) on C, Z = U^-1 Y.  Scaling, unlike eigx_gev_range (which does not scale B): each pencil by its
 * own maxima, both matrices, by exact powers of two -- A by the rule of eigx_s_batch (only when max|a| lies outside
 * [1e-90, 1e90]), B by the same rule with an even exponent, C once more after it is formed; w, z and U are unscaled exactly.
 * With A in range, B = I and C in range no step changes a bit: w and z are then those of eigx_s_batch.  No workgroup waits for
 * another.  The arithmetic of a pencil depends on n alone: the result at position k of a batch is bit for bit that of the
 * pencil solved alone, and two runs agree bit for bit.  n above the cutoff (eigx_tune key 23, default EIGX_GBATCH_NMAX): the
 * entry calls eigx_gev_range_dev(n, il = 1, iu = n, ..., mode) pencil by pencil, so every n and every leading dimension work
 * (a pencil with an odd lda, ldb or ldz is staged through pool buffers "gbatch.*" of even leading dimension); such a pencil
 * inherits that entry's behaviour: B is not scaled, and the not-positive-definite message is printed once per failed pencil.
 * The device form waits on the default stream on entry and returns after the result is complete.  eigx_get_timers [0] = the
 * seconds of the call, the rest 0.  Workspace: none beyond the status words (pool buffers "gbatch.*"); the host form stages a, b,
 * z and w through the pool buffers of the other host forms. */
#define EIGX_GBATCH_NMAX 96
int eigx_gev_batch(int n, int batch, double* a, int lda, int64_t stride_a, double* b, int ldb, int64_t stride_b, double* w, int ldw,
                   double* z, int ldz, int64_t stride_z, char mode, int* info);
int eigx_gev_batch_dev(int n, int batch, double* a_dev, int lda, int64_t stride_a, double* b_dev, int ldb, int64_t stride_b,
                       double* w_dev, int ldw, double* z_dev, int ldz, int64_t stride_z, char mode, int* info_dev);


#ifdef __cplusplus
}
#endif
#endif /* EIGENEXA_AMD_GBATCH_H */
