/* eigenexa_amd_gvbatch.h -- the ragged batched generalised eigensolves of libeigenexa_amd.so (an EXTENSION, not in the reference).
 * Part of the C-ABI of eigenexa_amd.h, which includes this file: include that header.  The entries have a file of their own
 * because the lists of entries of the other headers and the ctypes tables that mirror them (eigenexa_amd/_lib.py) are held fixed,
 * name by name, by their tests; these are mirrored by _lib.GVBATCH_SIGNATURES and held against it by tests/test_gvbatch.py in the
 * same way. */
#ifndef EIGENEXA_AMD_GVBATCH_H
#define EIGENEXA_AMD_GVBATCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Ragged batched generalised eigensolves -- EXTENSION, not in the reference: `batch` real symmetric-definite (eigx_gev_vbatch) or
 * complex Hermitian-definite (eigx_hgev_vbatch) pencils A x = lambda B x, every one with its own order, solved completely in one
 * call: the symmetry sectors of a block-diagonal Hamiltonian in a non-orthogonal basis, per-k-point blocks with an overlap
 * matrix.  The ragged siblings of eigx_gev_batch / eigx_hgev_batch, in the storage convention of eigx_s_vbatch / eigx_h_vbatch
 * (eigenexa_amd_vbatch.h) with b, off_b and ldb added.  One GPU only: with more than one rank the entries print the line of the
 * range entries and return EIGX_ERR_BAD_ARG.
 * Descriptors: n, off_a, lda, off_b, ldb, off_w, off_z and ldz are HOST arrays of `batch` entries in both forms.  Block k
 * (0-based) is the pencil (a + off_a[k], b + off_b[k]), column-major with the leading dimensions lda[k], ldb[k] and the order
 * n[k]; its eigenvalues come back in w + off_w[k], ascending; its eigenvectors in z + off_z[k] with the leading dimension ldz[k].
 * Offsets and leading dimensions count elements: doubles for eigx_gev_vbatch; COMPLEX elements for a, b and z of
 * eigx_hgev_vbatch, whose a, b and z are interleaved (re, im) doubles as for eigx_hgev_batch and whose w is real (off_w in
 * doubles).  Blocks must not overlap one another, in a, in b, in w or in z: this is the caller's responsibility and is not
 * checked.
 * Per block the contract is that of eigx_gev_batch / eigx_hgev_batch: of a and b only the upper triangles are read (of the
 * Hermitian diagonals only the real parts; the strict lower triangles, the rows beyond n[k] and whatever lies between the
 * blocks may hold anything, NaN included); a is destroyed; the upper triangle of the block of b returns U with B = U^T U /
 * U^H U for the caller's B, its diagonal real and positive (eigx_hgev_vbatch: the imaginary parts of the diagonal are written as
 * 0), the rest of b is left untouched; z is B-orthonormal, z^T B z = I / z^H B z = I; only w(1:n[k]) and z(1:n[k], 1:n[k]) of a
 * block are written.  mode 'A' eigenpairs, 'N' eigenvalues and U only (z, off_z and ldz may be NULL; w and U are bit for bit those
 * of mode 'A').  n[k] = 0 is an empty block: nothing of it is touched and info[k] = 0.  batch = 0 returns EIGX_OK.
 * EIGX_ERR_BAD_ARG, for the whole call and before anything runs: batch < 0; a mode other than 'A' / 'N'; with batch > 0 a NULL
 * among n, a, off_a, lda, b, off_b, ldb, w, off_w (b, off_b and ldb in both modes) and in mode 'A' among z, off_z, ldz; for some
 * k n[k] < 0, lda[k] < n[k], ldb[k] < n[k], off_a[k] < 0, off_b[k] < 0, off_w[k] < 0, or in mode 'A' ldz[k] < n[k] or
 * off_z[k] < 0.
 * Per-block status: info[k] = 0, EIGX_ERR_NONFINITE (a NaN / Inf in what is read of a or b: w of the block = NaN, its z and its b
 * untouched), EIGX_ERR_NOT_SPD (B is not positive definite, or too close to singular for U^-T A U^-1 to be formed: w = NaN, z
 * untouched; b untouched where a kernel served the block, else as eigx_gev_range / eigx_hgev_range leave it) or
 * EIGX_ERR_INTERNAL (the QL iteration used up its 30 n iterations: w = NaN, z and b unspecified).  info may be NULL; in the _dev
 * forms it is a device int array of `batch` entries.  A failed block never disturbs the others; the call returns EIGX_OK or the
 * code of the failed block with the lowest caller index k.
 * Method (csrc/gvbatch.hip, csrc/hgbatch.hip): the blocks with n[k] at or below the cutoff of the uniform
 * entry (eigx_tune key 23 for eigx_gev_vbatch, at most 96; key 24 for eigx_hgev_vbatch, at most 64) are sorted by n-class (32,
 * 64, 96) on the host (eigx_vbatch_plan), one descriptor per block is uploaded in one copy, and one launch per non-empty class,
 * largest first, solves them with one workgroup per block, both matrices in LDS from load to store, by the arithmetic of
 * eigx_gev_batch / eigx_hgev_batch: Cholesky of B, two triangular substitutions, reduction and QL, a back-substitution.  No
 * workgroup waits for another.  The arithmetic of a block depends on its n alone: w, z and U of block k are bit for bit those of
 * eigx_gev_batch_dev(n[k], 1, ...) / eigx_hgev_batch_dev(n[k], 1, ...) on the same pencil, whatever the other blocks are, in
 * whatever order, and from run to run.  A block above the cutoff goes through eigx_gev_range_dev / eigx_hgev_range_dev(n, 1, n,
 * ...) as in eigx_gev_batch / eigx_hgev_batch (a real block with an odd leading dimension through an even-ld copy) and inherits
 * that entry's behaviour; a status of it that belongs to no block (out of memory, ...) ends the call.  The device forms wait on
 * the default stream on entry and return after the result is complete.  eigx_get_timers [0] = the seconds of the call, the
 * rest 0.
 * The host forms stage of each of a, b, w and z the span from the lowest offset to the highest last element of a block
 * (off + ld (n - 1) + n) in one copy, through the pool buffers of the other host forms; the spans of b, w and z go up before the
 * solve and come back after it, so U returns, and gaps, padding and the z and b of a failed block return as they were passed. */
int eigx_gev_vbatch(int batch, const int* n, double* a, const int64_t* off_a, const int* lda, double* b, const int64_t* off_b,
                    const int* ldb, double* w, const int64_t* off_w, double* z, const int64_t* off_z, const int* ldz, char mode,
                    int* info);
int eigx_gev_vbatch_dev(int batch, const int* n, double* a_dev, const int64_t* off_a, const int* lda, double* b_dev,
                        const int64_t* off_b, const int* ldb, double* w_dev, const int64_t* off_w, double* z_dev, const int64_t* off_z,
                        const int* ldz, char mode, int* info_dev);
int eigx_hgev_vbatch(int batch, const int* n, double* a, const int64_t* off_a, const int* lda, double* b, const int64_t* off_b,
                     const int* ldb, double* w, const int64_t* off_w, double* z, const int64_t* off_z, const int* ldz, char mode,
                     int* info);
int eigx_hgev_vbatch_dev(int batch, const int* n, double* a_dev, const int64_t* off_a, const int* lda, double* b_dev,
                         const int64_t* off_b, const int* ldb, double* w_dev, const int64_t* off_w, double* z_dev,
                         const int64_t* off_z, const int* ldz, char mode, int* info_dev);

#ifdef __cplusplus
}
#endif
#endif /* EIGENEXA_AMD_GVBATCH_H */
