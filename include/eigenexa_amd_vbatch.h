/* eigenexa_amd_vbatch.h -- the ragged batched eigensolves of libeigenexa_amd.so (an EXTENSION, not in the reference).  Part of the
 * C-ABI of eigenexa_amd.h, which includes this file: include that header.  The entries have a file of their own because the list
 * of entries of eigenexa_amd.h and the ctypes table that mirrors it (eigenexa_amd/_lib.py, SIGNATURES) are held fixed, name by
 * name and in order, by tests/test_api_frontend.py; these are mirrored by _lib.VBATCH_SIGNATURES and held against it by
 * tests/test_vbatch.py in the same way. */
#ifndef EIGENEXA_AMD_VBATCH_H
#define EIGENEXA_AMD_VBATCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Ragged batched eigensolves -- EXTENSION, not in the reference: `batch` real symmetric (eigx_s_vbatch) or complex Hermitian
 * (eigx_h_vbatch) matrices, every one with its own order, solved completely in one call: the symmetry sectors of a block-diagonal
 * Hamiltonian, per-site density-matrix blocks, per-k-point blocks after a basis truncation.  One GPU only: with more than one
 * rank the entries print the line of the range entries and return EIGX_ERR_BAD_ARG.
 * Descriptors: n, off_a, lda, off_w, off_z and ldz are HOST arrays of `batch` entries in both forms (the caller knows its block
 * sizes on the host; the schedule is made there).  Block k (0-based) is a + off_a[k], column-major with the leading dimension
 * lda[k] and the order n[k]; its eigenvalues come back in w + off_w[k], ascending; its eigenvectors in z + off_z[k] with the
 * leading dimension ldz[k].  Offsets and leading dimensions count elements: doubles for eigx_s_vbatch; COMPLEX elements for a and
 * z of eigx_h_vbatch, whose a and z are interleaved (re, im) doubles as for eigx_h_batch and whose w is real (off_w in doubles).
 * Blocks must not overlap one another, in a, in w or in z: this is the caller's responsibility and is not checked.
 * Per block the contract is that of eigx_s_batch / eigx_h_batch: only the upper triangle is read (of a Hermitian diagonal only
 * the real parts; the strict lower triangle, the rows beyond n[k] and whatever lies between the blocks may hold anything, NaN
 * included); a is destroyed; only w(1:n[k]) and z(1:n[k], 1:n[k]) of a block are written: padding rows, gaps and everything
 * between the blocks are left untouched.  mode 'A' eigenpairs, 'N' eigenvalues only (z, off_z and ldz may be NULL; w is bit for
 * bit that of mode 'A').  n[k] = 0 is an empty block: nothing of it is touched and info[k] = 0.  batch = 0 returns EIGX_OK.
 * EIGX_ERR_BAD_ARG, for the whole call and before anything runs: batch < 0; a mode other than 'A' / 'N'; with batch > 0 a NULL
 * among n, a, off_a, lda, w, off_w and in mode 'A' among z, off_z, ldz; for some k n[k] < 0, lda[k] < n[k], off_a[k] < 0,
 * off_w[k] < 0, or in mode 'A' ldz[k] < n[k] or off_z[k] < 0.
 * Per-block status: info[k] = 0, EIGX_ERR_NONFINITE (a NaN / Inf in what is read: w of the block = NaN, its z untouched) or
 * EIGX_ERR_INTERNAL (the QL iteration used up its 30 n iterations: w = NaN, z unspecified).  info may be NULL; in the _dev forms
 * it is a device int array of `batch` entries.  A failed block never disturbs the others; the call returns EIGX_OK or the code
 * of the failed block with the lowest caller index k.
 * Method (csrc/vbatch.hip, csrc/hvbatch.hip): the blocks with n[k] at or below the cutoff of the uniform
 * entry (eigx_tune key 21 for eigx_s_vbatch, key 22 for eigx_h_vbatch) are sorted by n-class (32, 64, 96, 128) on the host
 * (eigx_vbatch_plan), one descriptor per block is uploaded in one copy, and one launch per non-empty class, largest first, solves
 * them with one workgroup per block, the block in LDS from load to store, by the arithmetic of eigx_s_batch / eigx_h_batch.  No
 * workgroup waits for another.  The arithmetic of a block depends on its n alone: w and z of block k are bit for bit those of
 * eigx_s_batch_dev(n[k], 1, ...) / eigx_h_batch_dev(n[k], 1, ...) on the same block, whatever the other blocks are, in whatever
 * order, and from run to run.  A block above the cutoff goes through eigx_s_dev / eigx_h_dev(n, nvec = n, ..., m_forward = 48,
 * m_backward = 128, mode) as in eigx_s_batch and inherits that entry's behaviour (its a(1:3, 1) / a(1:2, 1) statistics included);
 * a status of it that belongs to no block (out of memory, ...) ends the call.  The device forms wait on the default stream on
 * entry and return after the result is complete.  eigx_get_timers [0] = the seconds of the call, the rest 0.
 * The host forms stage of each of a, w and z the span from the lowest offset to the highest last element of a block
 * (off + ld (n - 1) + n) in one copy, through the pool buffers of the other host forms; the spans of w and z go up before the
 * solve and come back after it, so gaps, padding and the z of a failed block return as they were passed.  A caller whose
 * blocks are spread thinly over a large buffer pays for the span: pack them (eigenexa_amd.layout.ragged_offsets). */
int eigx_s_vbatch(int batch, const int* n, double* a, const int64_t* off_a, const int* lda, double* w, const int64_t* off_w, double* z,
                  const int64_t* off_z, const int* ldz, char mode, int* info);
int eigx_s_vbatch_dev(int batch, const int* n, double* a_dev, const int64_t* off_a, const int* lda, double* w_dev, const int64_t* off_w,
                      double* z_dev, const int64_t* off_z, const int* ldz, char mode, int* info_dev);
int eigx_h_vbatch(int batch, const int* n, double* a, const int64_t* off_a, const int* lda, double* w, const int64_t* off_w, double* z,
                  const int64_t* off_z, const int* ldz, char mode, int* info);
int eigx_h_vbatch_dev(int batch, const int* n, double* a_dev, const int64_t* off_a, const int* lda, double* w_dev, const int64_t* off_w,
                      double* z_dev, const int64_t* off_z, const int* ldz, char mode, int* info_dev);

/* The schedule of such a call; pure arithmetic, usable before eigx_init and without a GPU.  n: `batch` block sizes; cutoff: the
 * largest n the kernels serve (0 .. top); top: the family's largest n-class, 128 (eigx_s_vbatch) or 96 (eigx_h_vbatch: every n
 * above 64 takes the class of 96).  order (batch entries) receives a permutation of 0 .. batch-1: first the kernel-served blocks
 * (1 <= n[k] <= cutoff) by n-class from the largest class down, inside a class by descending n, ties by ascending index
 * (workgroups are handed out in index order, so the longest jobs start first); then the blocks above the cutoff by ascending
 * index; then the empty ones by ascending index.  counts6 = {class 32, class 64, class 96, class 128, above the cutoff, empty}.
 * EIGX_ERR_BAD_ARG for batch < 0, a negative size, a top other than 96 / 128, a cutoff outside 0 .. top or a NULL array that is
 * needed. */
int eigx_vbatch_plan(int batch, const int* n, int cutoff, int top, int* order, int* counts6);

#ifdef __cplusplus
}
#endif
#endif /* EIGENEXA_AMD_VBATCH_H */
