/* eigenexa_amd_hgbatch.h -- the batched small complex generalised eigensolves of libeigenexa_amd.so (an EXTENSION, not in the
 * reference).  Part of the C-ABI of eigenexa_amd.h, which includes this file: include that header.  The entries have a file of
 * their own because the list of entries of eigenexa_amd.h and the ctypes table that mirrors it (eigenexa_amd/_lib.py,
 * SIGNATURES) are held fixed, name by name and in order, by tests/test_api_frontend.py, and eigenexa_amd_gbatch.h with its table
 * by tests/test_gbatch.py; these are mirrored by _lib.HGBATCH_SIGNATURES and held against it by tests/test_hgbatch.py in the
 * same way. */
#ifndef EIGENEXA_AMD_HGBATCH_H
#define EIGENEXA_AMD_HGBATCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Batched small complex generalised eigensolves -- EXTENSION, not in the reference: `batch` Hermitian-definite pencils
 * A x = lambda B x of one size n, each solved completely (LAPACK callers know the per-pencil operation as zhegv, itype 1).  One
 * GPU only: with more than one rank the two entries print the line of the range entries and return EIGX_ERR_BAD_ARG.
 * The contract of eigx_gev_batch over complex numbers, on the storage of eigx_h_batch: a, b and z are interleaved (re, im)
 * doubles, column-major; lda, ldb, ldz, stride_a, stride_b and stride_z count COMPLEX elements; w is real.  Pencil k (0-based) is
 * a + k stride_a (leading dimension lda) and b + k stride_b (ldb); its eigenvalues come back in w + k ldw, ascending; its
 * eigenvectors in z + k stride_z (ldz), normalised so that z^H B z = I.  Only the upper triangles of a and b are read, and of
 * their diagonals only the real parts (the strict lower triangles, the imaginary parts of both diagonals, the rows beyond n and
 * the gaps may hold anything, NaN included); a is destroyed (contents unspecified, no statistics); a, b and z do not overlap.
 * Only w(1:n), z(1:n, 1:n) and the upper triangle of b of each pencil are written.  On exit, for a pencil with info[k] = 0, the
 * upper triangle of b(:, :, k) holds U with B = U^H U (the contract of eigx_hgev_range; U belongs to the caller's B, not to a
 * scaled copy), its diagonal real and positive with the imaginary parts written as exactly 0; the strict lower triangle of b,
 * its rows beyond n and the gaps are never written; the b of a pencil that failed is left as it was passed.
 * mode 'A' eigenpairs, 'N' eigenvalues only (z may be NULL; ldz and stride_z are ignored; U is still returned, and w and U are
 * bit for bit those of mode 'A'); anything else is EIGX_ERR_BAD_ARG.  EIGX_ERR_BAD_ARG also unless n >= 1, batch >= 0, lda >= n,
 * ldb >= n, ldw >= n, stride_a >= lda n and stride_b >= ldb n where batch > 1, b non-NULL, and in mode 'A' ldz >= n,
 * stride_z >= ldz n where batch > 1.  batch = 0 returns EIGX_OK and touches nothing.
 * Per-pencil status: info[k] = 0; EIGX_ERR_NONFINITE (a NaN / Inf in what is read of A or of B, both scanned before anything is
 * factored: w(:, k) = NaN, z(:, :, k) and b(:, :, k) untouched); EIGX_ERR_NOT_SPD (a Cholesky pivot that is not > 0 or not
 * finite, the rule of eigx_zchol_dev, or a non-finite entry in the formed C: w(:, k) = NaN, z(:, :, k) untouched, b as passed;
 * the batch kernel prints no message); or EIGX_ERR_INTERNAL (the QL iteration used up its 30 n iterations: w(:, k) = NaN,
 * z(:, :, k) unspecified).  info may be NULL; in the _dev form it is a device int array.  A failed pencil never disturbs the
 * others; the call returns EIGX_OK or the code of the failed pencil with the lowest index.
 * Method (csrc/hgbatch.hip): for n <= EIGX_HGBATCH_NMAX one launch, one workgroup per pencil, both matrices
 * as split planes in LDS from load to store: B = U^H U, C = U^-H A U^-1 by two triangular substitutions, the reduction, phase
 * chain and QL iteration of eigx_h_batch (the same arithmetic) on C, Z = U^-1 Y.  Scaling as in eigx_gev_batch: each pencil by
 * its own maxima of max(|Re|, |Im|), both matrices, by exact powers of two -- A only when its maximum lies outside
 * [1e-90, 1e90], B by the same rule with an even exponent, C once more after it is formed; w, z and U are unscaled exactly.
 * With A in range, B = I and C in range no step changes a bit: w and z are then those of eigx_h_batch.  No workgroup waits for
 * another.  The arithmetic of a pencil depends on n alone: the result at position k of a batch is bit for bit that of the
 * pencil solved alone, and two runs agree bit for bit.  n above the cutoff (eigx_tune key 24, default EIGX_HGBATCH_NMAX): the
 * entry calls eigx_hgev_range_dev(n, il = 1, iu = n, ..., mode) pencil by pencil, so every n and every leading dimension work;
 * such a pencil inherits that entry's behaviour: B is not scaled, and the not-positive-definite message is printed once per
 * failed pencil.  The device form waits on the default stream on entry and returns after the result is complete.
 * eigx_get_timers [0] = the seconds of the call, the rest 0.  Workspace: none beyond the status words; the host form stages a,
 * b, z and w through the pool buffers of the other complex host forms. */
#define EIGX_HGBATCH_NMAX 64
int eigx_hgev_batch(int n, int batch, double* a, int lda, int64_t stride_a, double* b, int ldb, int64_t stride_b, double* w, int ldw,
                    double* z, int ldz, int64_t stride_z, char mode, int* info);
int eigx_hgev_batch_dev(int n, int batch, double* a_dev, int lda, int64_t stride_a, double* b_dev, int ldb, int64_t stride_b,
                        double* w_dev, int ldw, double* z_dev, int ldz, int64_t stride_z, char mode, int* info_dev);


#ifdef __cplusplus
}
#endif
#endif /* EIGENEXA_AMD_HGBATCH_H */
