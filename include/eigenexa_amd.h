/* eigenexa_amd.h -- C-ABI of the MI355X-native EigenExa hot path (libeigenexa_amd.so).
 *
 * Plain C, plain pointers and sizes; no torch / HIP types in any signature (streams are the
 * library's own).  Every entry point names the reference interface it replaces
 * (paths relative to the RIKEN-RCCS/EigenExa 2.13 tree).
 *
 * Conventions kept from the reference:
 *   - all matrices column-major, fp64; indices/sizes 32-bit int;
 *   - the matrix is distributed 2-D cyclically (block size 1) over a Px x Py process grid,
 *     global (i,j) (0-based) -> rank (i%Px, j%Py), local (i/Px, j/Py)   (src/eigen_libs0.F:1825-2258);
 *   - only the upper triangle (global row <= global col) of `a` is read; `a` is destroyed and on
 *     return a(1,1)=flop count, a(2,1)=elapsed seconds, a(3,1)=communication seconds or -1
 *     (src/eigen_sx.F:285-296);
 *   - w(1:n) ascending eigenvalues, replicated; z(ldz, *) cyclic eigenvectors;
 *   - `mode`: only the first character is used: 'A' all eigenpairs, 'N' eigenvalues only,
 *     'X' eigenpairs + refined eigenvalues (src/eigen_sx.F:103-118).
 *   - errors: no status argument in the reference; here every function returns 0 on success and a
 *     negative code on a precondition failure (the Fortran module drops it to keep the
 *     reference's silent-return behaviour, src/eigen_sx.F:82-131).
 *
 * Two families of solver entry points:
 *   eigx_sx / eigx_s          host arrays in, host arrays out     (drop-in for the Fortran API)
 *   eigx_sx_dev / eigx_s_dev  device (HBM-resident) arrays        (what bench.py times)
 * and, on top of them: eigx_solve_bc[_dev] (block-cyclic local blocks of a ScaLAPACK descriptor),
 * eigx_gev[_dev] (KMATH_EIGEN_GEV), eigx_h[_dev] (complex Hermitian eigen_h), eigx_hgev[_dev] (KMATH_EIGEN_HGEV, an
 * extension: complex Hermitian generalised problem), eigx_sx_range / eigx_s_range[_dev] (an extension: eigenpairs il .. iu
 * of the ascending spectrum, one GPU), eigx_gev_range[_dev] (KMATH_EIGEN_GEV_RANGE, an extension: eigenpairs il .. iu of
 * the generalised problem by the Cholesky route, one GPU), eigx_hgev_range[_dev] (KMATH_EIGEN_HGEV_RANGE, an extension: the
 * same for the complex Hermitian generalised problem, one GPU), eigx_sx_range_v / eigx_s_range_v / eigx_gev_range_v[_dev] (an
 * extension: the eigenpairs with vl <= lambda < vu of the real solvers, LAPACK's range = 'V', one GPU), eigx_h_range[_v] and
 * eigx_hgev_range_v[_dev] (an extension: both kinds of window for the complex Hermitian solvers, one GPU), eigx_s_batch[_dev]
 * and eigx_h_batch[_dev] (an extension: many small symmetric / complex Hermitian matrices in one call, one GPU),
 * eigx_gev_batch[_dev] and eigx_hgev_batch[_dev] (an extension: many small symmetric-definite / Hermitian-definite pencils in
 * one call, one GPU), eigx_s_vbatch[_dev], eigx_h_vbatch[_dev], eigx_gev_vbatch[_dev] and eigx_hgev_vbatch[_dev] (an extension: the
 * same for blocks of differing sizes) and the stage
 * entry eigx_band_count_dev (Sturm counts of a band matrix at caller-given points).
 */
#ifndef EIGENEXA_AMD_H
#define EIGENEXA_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EIGX_OK 0
#define EIGX_ERR_NOT_INITIALIZED (-1)
#define EIGX_ERR_BAD_ARG (-2)
#define EIGX_ERR_TOO_LARGE (-3)
#define EIGX_ERR_NO_DEVICE (-4)
#define EIGX_ERR_NONFINITE (-5)
#define EIGX_ERR_INTERNAL (-6)
#define EIGX_ERR_NOT_SPD (-7)
#define EIGX_ERR_NO_MEMORY (-8)   /* a workspace allocation failed; on several ranks the others return EIGX_ERR_INTERNAL at once */
#define EIGX_ERR_WINDOW (-9)      /* a value window holds more eigenvalues than the caller gave room for (mmax); *m, *il are set */

/* ---- life cycle -------------------------------------------------------------------------- */

/* replaces eigen_init(comm, order)  src/eigen_libs.F:70-104 -> eigen_init0 src/eigen_libs0.F:296-376.
 * Single-rank form: 1x1 grid on HIP device `device`. */
int eigx_init(int device);

/* Multi-rank form (one process per GPU, all on one xGMI node).  `nranks` processes call this collectively; the
 * grid is Px = largest divisor of nranks <= sqrt(nranks), Py = nranks/Px, column-major rank order
 * (src/eigen_libs0.F:526-570).  `session_id` is the 128-byte id created by eigx_get_rccl_unique_id() on rank 0
 * and broadcast by the caller (MPI_Bcast in a Fortran/MPI host, torch.distributed in bench.py): an ncclUniqueId
 * when RCCL is installed (it also seeds the world / X / Y RCCL communicators), random bytes otherwise.  The ranks
 * find each other through a POSIX shared-memory board named after it, exchange hipIpcMemHandles of their
 * communication windows and map them: kernels then write into the peers' HBM over xGMI directly.
 * Replaces MPI_Comm_dup/MPI_Comm_split of eigen_init_comm_setup/eigen_init_cartesian_check,
 * src/eigen_libs0.F:382-428, :579-715.  Several ranks may share one GPU (the tests do): RCCL is then not used and
 * every collective goes through the peer windows.
 * Transport ladder, decided at init by a self-test with checksummed payloads on both transports (a few hundred
 * ready / push / flag / wait rounds and step-window rounds over the peer windows; all-reduces over the X, Y and world
 * RCCL communicators, all-gather and grouped send / receive): peer windows for everything if they pass (the form
 * every multi-rank test runs), RCCL for whatever they cannot carry (the per-step exchange then is one ncclAllGather
 * of the step messages -- the reference's reduce_dbl over X and Y, src/comm.F:1192-1247, as one collective), an error
 * return if neither works (bench.py then runs independent replicas).  eigx_comm_info reports what was chosen.
 * Environment: EIGX_COMM_TIMEOUT_S (default 120) bounds every wait for a peer; EIGX_BULK=rccl moves the bulk
 * collectives to RCCL; EIGX_STEP=coll selects the collective form of the per-step exchange; EIGX_FUSE_WAIT=1 folds the
 * step wait into the consumer kernel; EIGX_NO_IPC / EIGX_NO_RCCL disable a transport; EIGX_SELFTEST_ROUNDS (default 400,
 * 0 = skip), EIGX_SELFTEST_FAIL=ipc|rccl (make that leg report failure: tests of the ladder). */
int eigx_init_multi(int device, int rank, int nranks, const void* session_id, char order);
/* visible HIP devices (0 without a GPU): lets an MPI host map its node-local rank to a device
 * (eigen_libs_mod.F90: MPI_Comm_split_type + modulo) */
int eigx_get_device_count(void);
int eigx_get_rccl_unique_id(void* out128);
/* Explicit Px x Py process grid for the NEXT eigx_init_multi call (one-shot; 0, 0 clears): the 2-D cartesian
 * communicator form of eigen_init (eigen_init_cartesian_check, src/eigen_libs0.F:579-715), which the reference's
 * benchmark driver builds for its -x option (benchmark/main2.f:193-211). */
int eigx_set_grid_dims(int px, int py);

/* replaces eigen_get_comm src/eigen_libs0.F:1655-1669 as far as a GPU library can: what the caller needs to build
 * its own row / column communicators -- the colour and key of this rank in the X group (ranks sharing my column
 * coordinate: colour = y_id, key = x_id) and in the Y group (colour = x_id, key = y_id), 1-based ids. */
int eigx_get_comm(int* x_color, int* x_key, int* y_color, int* y_key);

/* Seconds this rank spent in communication (pushes, waits for peers, RCCL calls) during the last solve:
 * the a(3,1) statistic of src/eigen_sx.F:285-296 and the "COMM_STAT" tables of src/eigen_devel.F:364-526. */
double eigx_comm_seconds(void);

/* JSON text describing the transports in use (per-step exchange, its wait, bulk collectives) and the counts / errors /
 * microseconds per round of the init-time self-test, plus calls and bytes sent per kind of collective since init (the
 * reference's COMM_STAT tables, src/eigen_devel.F:364-526); "{"ranks": 1}" on one GPU.  The reference prints the analogous
 * communicator facts at init (src/eigen_libs0.F:774-1109 measures its collectives there). */
int eigx_comm_info(char* buf, int len);

/* 1-rank RCCL self-test (dlopen, communicator from a unique id, ncclCommSplit, allreduce / allgather / send-recv on
 * the library stream): validates the RCCL plumbing on a one-GPU box.  Returns 0 on success. */
int eigx_rccl_selftest(void);

/* replaces eigen_free  src/eigen_libs.F:204-216 */
int eigx_free(void);

/* replaces eigen_get_version src/eigen_libs0.F:175 ; version = 100*major+minor of this library */
int eigx_get_version(int* version, char* date32, char* vcode32);

/* replaces eigen_get_procs / eigen_get_id  src/eigen_libs0.F:1575-1655 (1-based ids like the reference) */
int eigx_get_procs(int* procs, int* x_procs, int* y_procs);
int eigx_get_id(int* id, int* x_id, int* y_id);

/* replaces eigen_get_errinfo src/eigen_libs0.F:1689-1698 */
int eigx_get_errinfo(int64_t* info);

/* replaces eigen_get_matdims(n, nx, ny, m_forward, m_backward, mode) src/eigen_libs.F:106-148,
 * src/eigen_libs0.F:1254-1371.  Returns local array extents that are >= the reference's for the
 * same (n, grid) so existing callers' allocations stay valid; nx = ny = -1 if too large.
 * Mode 'O' (the default): where the reference nudges nx off A64FX cache-set aliasing (src/CSTAB.F:73-131), nx here is
 * moved off MI355X memory-channel aliasing -- from 2048 on, nx mod 2048 lies in [512, 1536] (consecutive columns
 * 4 - 12 KiB apart modulo 16 KiB); the solvers work in place on a(nx, *), and this is worth 2 - 9 % of a solve. */
int eigx_get_matdims(int n, int* nx, int* ny, int m_forward, int m_backward, char mode);
/* the same rule for an explicit x_procs x y_procs grid; pure arithmetic (usable before eigx_init, without a GPU) */
int eigx_matdims_for_grid(int n, int x_procs, int y_procs, int m_forward, int m_backward, char mode, int* nx, int* ny);

/* replaces eigen_memory_internal src/eigen_libs0.F:1395-1549: bytes of device workspace a solve needs.  It covers the
 * reference's solvers (eigx_sx / eigx_s); the index-range extension keeps its own pooled buffers ("sub.": inverse-iteration
 * scratch of at most min(4 GiB, 8 n^2) bytes, about 2 n m + 2 m^2 doubles of bases, n iu doubles on a fallback with il > 1)
 * on top of whatever earlier solves left in the pool, which never shrinks before eigx_free. */
int64_t eigx_memory_internal(int n, int lda, int ldz, int m_forward, int m_backward);
/* bytes of device memory the library holds right now (pooled workspace + communication windows); the tests check it
 * against eigx_memory_internal and that it scales like 1/P on several ranks.  -1 before eigx_init. */
int64_t eigx_held_bytes(void);
/* the same for the pooled workspace buffers whose name starts with `prefix` (e.g. "gev." = what KMATH_EIGEN_GEV holds
 * beside the two eigen_s solves: the tests check that it is a few n^2 / P, nothing gathered).  -1 before eigx_init. */
int64_t eigx_held_bytes_named(const char* prefix);
/* pure arithmetic, no GPU needed: the pieces of the distributed transpose Z = A^T on the 2-D cyclic layout (the PDTRAN of
 * src/KMATH_EIGEN_GEV_1.F:57) that rank (px, py) of a Px x Py grid exchanges with rank (qx, qy).  A piece is the set of
 * elements Z(i, j) = A(j, i) with i = i0 + t step, j = j0 + u step (step = lcm(Px, Py)); send_*: the piece I pack for
 * (qx, qy), recv_*: the one I get from it; i0 or j0 = -1: that pair exchanges nothing.  The CPU tests assemble A^T from
 * the pieces for every grid up to 8 ranks. */
int eigx_transpose_plan(int x_procs, int y_procs, int px, int py, int qx, int qy, int* send_i0, int* send_j0, int* recv_i0,
                        int* recv_j0, int* step);

/* ---- index helpers (pure functions; 1-based like the reference, src/eigen_libs0.F:1744-2356) - */
int eigx_loop_start(int istart, int nnod, int inod);
int eigx_loop_end(int iend, int nnod, int inod);
int eigx_translate_l2g(int ictr, int nnod, int inod);
int eigx_translate_g2l(int ictr, int nnod, int inod);
int eigx_owner_node(int ictr, int nnod, int inod);
int eigx_owner_index(int ictr, int nnod, int inod);

/* ---- solvers ------------------------------------------------------------------------------ */

/* replaces eigen_sx(n,nvec,a,lda,w,z,ldz,m_forward,m_backward,mode) src/eigen_sx.F:30-308
 * (pentadiagonal route: eigen_prd -> eigen_dcx -> eigen_common_trbakwy(nb=2)). Host arrays. */
int eigx_sx(int n, int nvec, double* a, int lda, double* w, double* z, int ldz, int m_forward,
            int m_backward, char mode);

/* replaces eigen_s(...) src/eigen_libs.F:150-202 -> eigen_FS src/eigen_FS.F:29-300 /
 * eigen_s0 src/eigen_s.F:30-307 (tridiagonal route: eigen_trd -> dc2 -> trbakwy(nb=1)). Host arrays. */
int eigx_s(int n, int nvec, double* a, int lda, double* w, double* z, int ldz, int m_forward,
           int m_backward, char mode);

/* Same solvers on device-resident arrays (a_dev, w_dev, z_dev are HBM pointers of this rank's GPU).  lda >= the local
 * row count (any parity: an odd lda or a base that is not 16-byte aligned is served from an internal padded copy); like
 * the reference `a` is destroyed, and its padding rows (local rows beyond the matrix, up to lda) are scratch as well. */
/* Device entry points synchronise the (legacy) default stream on entry, so whatever the caller queued there to fill
 * the arguments is complete; a caller that fills them on another stream synchronises that stream itself.  They return
 * after the result is complete. */
int eigx_sx_dev(int n, int nvec, double* a_dev, int lda, double* w_dev, double* z_dev, int ldz,
                int m_forward, int m_backward, char mode);
int eigx_s_dev(int n, int nvec, double* a_dev, int lda, double* w_dev, double* z_dev, int ldz,
               int m_forward, int m_backward, char mode);

/* Index-range solves -- EXTENSION, not in the reference (whose nvec only trims the back-transformation and always means
 * "the lowest nvec"; LAPACK callers know this as range = 'I', il, iu).  One GPU only: with more than one rank the four
 * entries print one line and return EIGX_ERR_BAD_ARG.  il, iu are 1-based and inclusive, 1 <= il <= iu <= n,
 * m = iu - il + 1; on return w(1:m) holds eigenvalues il .. iu of the ascending spectrum and z(:, 1:m) the matching
 * orthonormal eigenvectors; w and z need room for m entries / columns only, nothing beyond is touched.  mode 'A'
 * eigenpairs, 'N' eigenvalues only (z untouched, may be NULL); anything else is EIGX_ERR_BAD_ARG.  a as for eigx_sx: upper
 * triangle read, destroyed, a(1:3,1) = flops / seconds / -1; same scaling, NaN / Inf check (w(1:m) = NaN,
 * EIGX_ERR_NONFINITE), odd-lda copy and wait on the default stream.
 * Method (csrc/subset.hip): band reduction as for eigx_sx / eigx_s, Sturm multi-section on the index
 * window, inverse iteration on the band matrix with one eigenvector per GPU thread, CholQR2 and Rayleigh-Ritz through the
 * fp64 MFMA GEMM, back-transformation of the m columns.  Work and workspace after the reduction scale with m; no D&C
 * workspace of size n is requested.  Fallback rule: when the acceptance test of the stage refuses its result (Cholesky
 * breakdown, or cond(L) above 10^key19), or when 100 m > key17 n (the size rule), the full divide and conquer computes the
 * lowest iu pairs and columns il .. iu are returned: the caller always gets a result that meets the reference's gates. */
int eigx_sx_range(int n, int il, int iu, double* a, int lda, double* w, double* z, int ldz, int m_forward, int m_backward,
                  char mode);
int eigx_s_range(int n, int il, int iu, double* a, int lda, double* w, double* z, int ldz, int m_forward, int m_backward,
                 char mode);
int eigx_sx_range_dev(int n, int il, int iu, double* a, int lda, double* w, double* z, int ldz, int m_forward,
                      int m_backward, char mode);
int eigx_s_range_dev(int n, int il, int iu, double* a, int lda, double* w, double* z, int ldz, int m_forward, int m_backward,
                     char mode);
/* the last range call: path 1 = subset path, 2 = fell back to the full D&C, 3 = full D&C by the size rule; m; cond = the
 * conditioning estimate max / min diag(L) of the acceptance test (0 when it did not run).  Any pointer may be NULL.  Only
 * the four solver entries, their value-window forms (path 0: the window was empty, did not fit, or only the count was asked
 * for), eigx_gev_range[_v][_dev] (for their inner call on C) and eigx_sx / eigx_s routed by key 18 write this record; the
 * stage entries do not. */
int eigx_range_info(int* path, int* m, double* cond);
/* stage seconds of the last range call: [0] bisection [1] inverse iteration [2] orthonormalisation + Rayleigh-Ritz (or
 * the fallback D&C) [3] back-transformation (tools/gpu_range_time.py) */
int eigx_range_timers(double* out4);

/* Value-window solves -- EXTENSION, not in the reference (LAPACK callers know this as range = 'V', vl, vu): the eigenpairs
 * with vl <= lambda < vu, without knowing their indices.  The contract of the index-range entries above with these changes.
 * One GPU only (the same printed line and EIGX_ERR_BAD_ARG on several ranks).
 * Window: half-open, as the library's Sturm count (eigenvalues below x) defines it; an eigenvalue within rounding of an
 * end point may fall on either side, as in LAPACK.  vl = -Inf and vu = +Inf are allowed and cost no count.  After the band
 * reduction (once: no second reduction as with a mode-'N' solve followed by an index call) two counts at sigma vl,
 * sigma vu (sigma = the scale factor of eigen_scaling; a matrix of scale 1e120 works) give il = count(vl) + 1,
 * iu = count(vu), m = max(0, iu - il + 1); the counts use the Sturm sequence and pivmin of the multi-section, so the window
 * agrees with the brackets the multi-section then builds for il .. iu.  From there the call runs the code of the index
 * call il .. iu: size rule (key 17), acceptance test (key 19), fallback, eigx_range_info, eigx_range_timers and a(1:3,1)
 * stay in force, and w, z are bit-identical to that call's.
 * mmax = room in w (entries) and z (columns); *m and *il (host pointers in the host AND the device forms) receive the
 * number of eigenvalues in the window and the 1-based index of the first.  On return w(1:m), z(:, 1:m); nothing beyond m
 * entries / columns is touched.
 *   m = 0:      EIGX_OK, *m = 0, *il = count(vl) + 1; w, z untouched, no eigenvector stage, no back-transformation;
 *               eigx_range_info: path 0, m 0; a(1:3,1) is written.
 *   m > mmax:   EIGX_ERR_WINDOW, *m and *il set, w, z untouched, the rest of the solve does not run; the caller retries
 *               through the index entries with il .. il + m - 1 (host forms: a is untouched; device forms: a is destroyed,
 *               as in every other case).
 *   mode 'C':   count only (value form only): *m, *il as above and return; w, z may be NULL, mmax is ignored; the cost is
 *               one reduction; a(1:3,1) is written.  Modes 'A' and 'N' as for the index entries.
 * EIGX_ERR_BAD_ARG unless vl < vu (a NaN bound fails it), mmax >= 1 (not for mode 'C'), m and il non-NULL, and the rest as
 * for the index entries with mmax in the place of iu - il + 1.  NaN / Inf in the upper triangle: EIGX_ERR_NONFINITE,
 * w(1:mmax) = NaN, *m = 0. */
int eigx_sx_range_v(int n, double vl, double vu, int mmax, int* m, int* il, double* a, int lda, double* w, double* z, int ldz,
                    int m_forward, int m_backward, char mode);
int eigx_s_range_v(int n, double vl, double vu, int mmax, int* m, int* il, double* a, int lda, double* w, double* z, int ldz,
                   int m_forward, int m_backward, char mode);
int eigx_sx_range_v_dev(int n, double vl, double vu, int mmax, int* m, int* il, double* a, int lda, double* w, double* z,
                        int ldz, int m_forward, int m_backward, char mode);
int eigx_s_range_v_dev(int n, double vl, double vu, int mmax, int* m, int* il, double* a, int lda, double* w, double* z,
                       int ldz, int m_forward, int m_backward, char mode);

/* Batched small symmetric eigensolves -- EXTENSION, not in the reference (which solves one large matrix per call): `batch`
 * symmetric matrices of one size n, each solved completely (LAPACK callers know the per-matrix operation as dsyev; vendor
 * libraries call this form "strided batched").  One GPU only: with more than one rank the two entries print the line of the
 * range entries and return EIGX_ERR_BAD_ARG.
 * Storage: matrix k (0-based) is a + k stride_a, column-major with leading dimension lda; its eigenvalues come back in
 * w + k ldw, ascending; its orthonormal eigenvectors in z + k stride_z with leading dimension ldz.  Strides and leading
 * dimensions are in doubles.  The upper triangle of each matrix is significant (the strict lower triangle and the rows
 * beyond n may hold anything, NaN included); a is destroyed (contents unspecified, no statistics); a and z do not overlap.
 * Only w(1:n) and z(1:n, 1:n) of each matrix are written: rows of z beyond n, entries of w beyond n and the gaps between
 * matrices are left untouched.
 * mode 'A' eigenpairs, 'N' eigenvalues only (z may be NULL; ldz and stride_z are ignored); anything else is
 * EIGX_ERR_BAD_ARG.  EIGX_ERR_BAD_ARG also unless n >= 1, batch >= 0, lda >= n, ldw >= n, stride_a >= lda n where batch > 1,
 * and in mode 'A' ldz >= n, stride_z >= ldz n where batch > 1.  batch = 0 returns EIGX_OK and touches nothing.
 * Per-matrix status: info[k] = 0, EIGX_ERR_NONFINITE (a NaN / Inf in the upper triangle: w(:, k) = NaN, z(:, :, k) untouched)
 * or EIGX_ERR_INTERNAL (the QL iteration used up its 30 n iterations, the budget of LAPACK's dsteqr: w(:, k) = NaN,
 * z(:, :, k) unspecified).  info may be NULL; in the _dev form it is a device int array.  A failed matrix never disturbs the others;
 * the call returns EIGX_OK or the code of the failed matrix with the lowest index.
 * Method (csrc/batch.hip): for n <= EIGX_BATCH_NMAX one launch, one workgroup per matrix, the matrix in
 * LDS from load to store: scaling by the rule of eigx_sx (each matrix by its own max|a|; scales of 1e120 and 1e-120 may sit
 * in one batch), Householder tridiagonalisation with Q accumulated in place, implicit QL with Wilkinson shift, sort.  No
 * workgroup waits for another.  The arithmetic of a matrix depends on n alone: the result at position k of a batch is bit
 * for bit that of the matrix solved alone, and two runs agree bit for bit.  n above the cutoff (eigx_tune key 21, default
 * EIGX_BATCH_NMAX): the entry calls eigx_s_dev(n, nvec = n, ..., m_forward = 48, m_backward = 128, mode) matrix by matrix,
 * so every n works and such a matrix gets the result (a(1:3,1) included) that eigx_s_dev gives.
 * The device form waits on the default stream on entry and returns after the result is complete.  eigx_get_timers [0] = the
 * seconds of the call, the rest 0.  Workspace: none beyond the status words (pool buffers "batch.*"); the host form stages
 * a, z and w through the pool buffers of the other host forms. */
#define EIGX_BATCH_NMAX 128
int eigx_s_batch(int n, int batch, double* a, int lda, int64_t stride_a, double* w, int ldw, double* z, int ldz,
                 int64_t stride_z, char mode, int* info);
int eigx_s_batch_dev(int n, int batch, double* a_dev, int lda, int64_t stride_a, double* w_dev, int ldw, double* z_dev, int ldz,
                     int64_t stride_z, char mode, int* info_dev);

/* Batched small complex Hermitian eigensolves -- EXTENSION, not in the reference: the complex sibling of eigx_s_batch (LAPACK
 * callers know the per-matrix operation as zheev).  `batch` Hermitian matrices of one size n, each solved completely.  One
 * GPU only: with more than one rank the two entries print the line of the range entries and return EIGX_ERR_BAD_ARG.
 * Storage: a and z hold interleaved (re, im) doubles as for eigx_h; lda, ldz, stride_a and stride_z are in COMPLEX elements
 * (matrix k starts at the double a + 2 k stride_a, its eigenvectors at z + 2 k stride_z); w is real, the ascending eigenvalues
 * of matrix k in w + k ldw.  The upper triangle of each matrix is significant, and of the diagonal the real parts only: the
 * strict lower triangle, the imaginary parts of the diagonal and the rows beyond n may hold anything, NaN included.  a is
 * destroyed (contents unspecified, no statistics); a and z do not overlap.  Only w(1:n) and z(1:n, 1:n) of each matrix are
 * written: rows of z beyond n, entries of w beyond n and the gaps between matrices are left untouched.  The eigenvectors are
 * orthonormal (z^H z = I); their phases are whatever the method leaves.
 * mode, the argument rules, batch = 0, info and the return value are exactly those of eigx_s_batch: 'A' eigenpairs, 'N'
 * eigenvalues only (z may be NULL; ldz and stride_z are ignored); EIGX_ERR_BAD_ARG unless n >= 1, batch >= 0, lda >= n,
 * ldw >= n, stride_a >= lda n where batch > 1, and in mode 'A' ldz >= n, stride_z >= ldz n where batch > 1; batch = 0 returns
 * EIGX_OK and touches nothing; info[k] = 0, EIGX_ERR_NONFINITE (a NaN / Inf in what is read of matrix k: w(:, k) = NaN,
 * z(:, :, k) untouched) or EIGX_ERR_INTERNAL (the QL iteration used up its 30 n iterations: w(:, k) = NaN, z(:, :, k)
 * unspecified); info may be NULL, in the _dev form it is a device int array; a failed matrix never disturbs the others and the
 * call returns EIGX_OK or the code of the failed matrix with the lowest index.
 * Method (csrc/hbatch.hip): for n <= EIGX_HBATCH_NMAX one launch, one workgroup per matrix, the matrix as
 * split real / imaginary planes in LDS from load to store: scaling by the rule of eigx_sx (each matrix by its own largest
 * |Re|, |Im|), Householder tridiagonalisation with Hermitian reflectors to a Hermitian tridiagonal matrix, a chain of unit
 * phases that makes it real (folded into the accumulated Q), implicit QL with Wilkinson shift on the real tridiagonal matrix,
 * sort.  No workgroup waits for another.  The arithmetic of a matrix depends on n alone: the result at position k of a batch
 * is bit for bit that of the matrix solved alone, and two runs agree bit for bit.  n above the cutoff (eigx_tune key 22,
 * default EIGX_HBATCH_NMAX): the entry calls eigx_h_dev(n, nvec = n, ..., m_forward = 48, m_backward = 128, mode) matrix by
 * matrix, so every n works and such a matrix gets the result (a(1:2,1) included) that eigx_h_dev gives.
 * The device form waits on the default stream on entry and returns after the result is complete.  eigx_get_timers [0] = the
 * seconds of the call, the rest 0.  Workspace: none beyond the status words (pool buffers "hbatch.*"); the host form stages
 * a, z and w through the pool buffers of the other complex host forms. */
#define EIGX_HBATCH_NMAX 96
int eigx_h_batch(int n, int batch, double* a, int lda, int64_t stride_a, double* w, int ldw, double* z, int ldz,
                 int64_t stride_z, char mode, int* info);
int eigx_h_batch_dev(int n, int batch, double* a_dev, int lda, int64_t stride_a, double* w_dev, int ldw, double* z_dev, int ldz,
                     int64_t stride_z, char mode, int* info_dev);

/* Batched small generalised eigensolves eigx_gev_batch[_dev] -- EXTENSION, not in the reference: declared and documented in
 * eigenexa_amd_gbatch.h beside this file, which comes in here, so this header alone still gives a caller the whole interface. */
#include "eigenexa_amd_gbatch.h"
/* The same over complex numbers, eigx_hgev_batch[_dev] -- EXTENSION: declared and documented in eigenexa_amd_hgbatch.h. */
#include "eigenexa_amd_hgbatch.h"
/* Ragged batches, eigx_s_vbatch[_dev] and eigx_h_vbatch[_dev] with their schedule eigx_vbatch_plan -- EXTENSION: declared and
 * documented in eigenexa_amd_vbatch.h. */
#include "eigenexa_amd_vbatch.h"
/* Ragged batches of pencils, eigx_gev_vbatch[_dev] and eigx_hgev_vbatch[_dev] -- EXTENSION: declared and documented in
 * eigenexa_amd_gvbatch.h. */
#include "eigenexa_amd_gvbatch.h"
/* Windowed batches, eigx_s_batch_range[_dev] with eigx_batch_range_info: eigenpairs il .. iu of every matrix of a batch --
 * EXTENSION: declared and documented in eigenexa_amd_batch_range.h. */
#include "eigenexa_amd_batch_range.h"
/* Windowed Hermitian batches, eigx_h_batch_range[_dev]: the same for complex Hermitian matrices -- EXTENSION: declared and
 * documented in eigenexa_amd_hbatch_range.h. */
#include "eigenexa_amd_hbatch_range.h"
/* Windowed batches of pencils, eigx_gev_batch_range[_dev]: eigenpairs il .. iu of every symmetric-definite pencil of a batch --
 * EXTENSION: declared and documented in eigenexa_amd_gbatch_range.h. */
#include "eigenexa_amd_gbatch_range.h"
/* Windowed batches of complex pencils, eigx_hgev_batch_range[_dev]: eigenpairs il .. iu of every Hermitian-definite pencil of a
 * batch -- EXTENSION: declared and documented in eigenexa_amd_hgbatch_range.h. */
#include "eigenexa_amd_hgbatch_range.h"

/* ScaLAPACK interop without a redistribution step.  The reference asks block-cyclic callers to
 * convert with pdgemr2d into its cyclic layout first (manual 3.4; benchmark/ev_test.f:68-84 does the reverse for the
 * check).  Here the layout is only an index map at the entry and exit of the solver, so the local blocks of a
 * descriptor with MB = NB = nb, RSRC = CSRC = 0 on the eigx process grid (eigx_get_procs / eigx_get_id, same grid
 * as a BLACS grid of that shape and order) are accepted as they are: a is the local numroc(n,nb,px,Px) x
 * numroc(n,nb,py,Py) block, z comes back as the local block of the n x nvec eigenvector matrix in the same
 * distribution, w replicated.  route: 2 = eigen_sx, 1 = eigen_s.  nb = 1 is the cyclic layout of eigx_sx / eigx_s. */
int eigx_solve_bc(int route, int n, int nvec, double* a, int lda, double* w, double* z, int ldz, int nb,
                  int m_forward, int m_backward, char mode);
int eigx_solve_bc_dev(int route, int n, int nvec, double* a_dev, int lda, double* w_dev, double* z_dev, int ldz,
                      int nb, int m_forward, int m_backward, char mode);
/* NUMROC(n, nb, iproc, 0, nprocs) of ScaLAPACK (TOOLS/numroc.f): local extent; -1 for invalid arguments */
int eigx_numroc(int n, int nb, int iproc, int nprocs);

/* replaces eigen_h(n,nvec,a,lda,w,z,ldz,m_forward,m_backward,mode) src/eigen_h.F:30-322 (complex Hermitian:
 * eigen_scaling_h -> eigen_hrd -> dc2 -> eigen_hrbakwyx).  a, z are complex(8) arrays passed as interleaved (re, im)
 * doubles, column-major, lda / ldz in COMPLEX elements; upper triangle of a significant; a is destroyed
 * (a(1,1) = flops, a(2,1) = seconds); w real, ascending; z = eigenvectors (unitary).  mode 'A', 'N', 'X'.  With more
 * than one rank a and z are the 2-D cyclic local blocks as for eigx_sx; the blocks are gathered and every rank solves
 * the replicated problem in this version (first cut: see csrc/herm.hip). */
int eigx_h(int n, int nvec, double* a, int lda, double* w, double* z, int ldz, int m_forward, int m_backward, char mode);
int eigx_h_dev(int n, int nvec, double* a_dev, int lda, double* w_dev, double* z_dev, int ldz, int m_forward,
               int m_backward, char mode);
/* eigen_h range solves -- EXTENSION, not in the reference (csrc/herm.hip herm_range_dev): eigenpairs
 * il .. iu of the ascending spectrum of a complex Hermitian matrix (eigx_h_range), or those with vl <= lambda < vu
 * (eigx_h_range_v).  The contracts of eigx_s_range and eigx_s_range_v above, word for word, on the storage of eigx_h: a, z
 * complex(8) as interleaved (re, im) doubles, lda / ldz in COMPLEX elements, upper triangle of a significant (Im of the
 * diagonal ignored), a destroyed with a(1,1) = flops, a(2,1) = seconds; w real.  One GPU only: with more than one rank
 * the entries print one line and return EIGX_ERR_BAD_ARG.  mode 'A' eigenpairs, 'N' eigenvalues only (z may be NULL), by
 * value also 'C' (count only); eigen_h's modes 'X' and 'S' are not offered (EIGX_ERR_BAD_ARG).  w(1:m), z(:, 1:m) with
 * z^H z = I_m; nothing beyond m entries / columns is touched.  NaN / Inf in the significant triangle: EIGX_ERR_NONFINITE,
 * w(1:m) (by value: w(1:mmax)) = NaN, *m = 0.  By value: the half-open window, mmax, *m, *il (host pointers in the host AND
 * the device forms), m = 0, EIGX_ERR_WINDOW and mode 'C' exactly as for eigx_s_range_v; the window is resolved on the real
 * tridiagonal matrix of eigen_hrd after ONE reduction, and w, z are bit-identical to the index call il .. iu.
 * Method: eigen_scaling_h, eigen_hrd and the T factors as eigx_h -> Sturm multi-section on the window -> inverse iteration
 * + CholQR2 + Rayleigh-Ritz on the real tridiagonal matrix (csrc/subset.hip, written straight into the real plane of m
 * columns; path 1) or the full divide and conquer with nvec = iu, of which the window is a pointer offset (path 3 by the
 * size rule of key 17, path 2 after a refusal by the acceptance test of key 19) -> eigen_hrbakwyx on the m columns.
 * eigx_range_info / eigx_range_timers are written as by the real range entries; eigx_get_timers as by eigx_h.  Inherits
 * eigen_h's overflow above a matrix scale of about 1e77. */
int eigx_h_range(int n, int il, int iu, double* a, int lda, double* w, double* z, int ldz, int m_forward, int m_backward,
                 char mode);
int eigx_h_range_dev(int n, int il, int iu, double* a_dev, int lda, double* w_dev, double* z_dev, int ldz, int m_forward,
                     int m_backward, char mode);
int eigx_h_range_v(int n, double vl, double vu, int mmax, int* m, int* il, double* a, int lda, double* w, double* z, int ldz,
                   int m_forward, int m_backward, char mode);
int eigx_h_range_v_dev(int n, double vl, double vu, int mmax, int* m, int* il, double* a_dev, int lda, double* w_dev,
                       double* z_dev, int ldz, int m_forward, int m_backward, char mode);

/* ---- stage entry points (device arrays; used by the parity tests and the profiler) ---------- */

/* replaces eigen_trd(n,a,lda,d,e,m) src/eigen_trd.F:82-113 (band=1) and
 * eigen_prd(n,a,lda,d,e,nme,m) src/eigen_prd.F:80-115 (band=2).
 * Out: d_dev[n]; e_dev[band*lde] with e(i,b) = band entry T(i-b,i) (1-based, zero for i<=b);
 * reflectors stay in a_dev columns, their 1/beta recoverable from e (src/trbakwy4.F:309-335). */
int eigx_band_reduce_dev(int n, double* a_dev, int lda, double* d_dev, double* e_dev, int lde,
                         int m_forward, int band);

/* replaces eigen_dc2 src/dc2.F (band=1) / eigen_dcx src/dcx.F:81-337 (band=2): eigen-decomposition of
 * the symmetric band matrix (d,e); w_dev ascending, z_dev(ldz, n) eigenvectors. */
int eigx_band_dc_dev(int n, int nvec, const double* d_dev, const double* e_dev, int lde, int band,
                     double* w_dev, double* z_dev, int ldz);

/* replaces KMATH_EIGEN_GEV(n,a,lda,b,ldb,w,z,ldz) src/KMATH_EIGEN_GEV.F:1-64 (-> KMATH_EIGEN_GEV_1.F:1-159): generalised
 * symmetric-definite problem A x = lambda B x through two eigen_s solves and three GEMMs.  Upper triangles of a, b
 * significant; w ascending; z B-orthonormal (z^T B z = I); a, b destroyed.  EIGX_ERR_NOT_SPD if B is not positive
 * definite (the reference prints "Matrix B is not positive definite!" and returns).  Host / device-resident arrays;
 * leading dimensions of the device form must be even.  Several ranks: a, b, z are the ranks' 2-D cyclic blocks as for
 * eigx_sx; first version: the blocks are gathered and every rank solves the replicated problem (the reference's is
 * distributed, src/KMATH_EIGEN_GEV_1.F:57-139). */
int eigx_gev(int n, double* a, int lda, double* b, int ldb, double* w, double* z, int ldz);
int eigx_gev_dev(int n, double* a_dev, int lda, double* b_dev, int ldb, double* w_dev, double* z_dev, int ldz);

/* KMATH_EIGEN_HGEV -- EXTENSION, not in the reference (which has no complex generalised solver): the complex
 * Hermitian-definite problem A x = lambda B x by the reference's method for the real case (src/KMATH_EIGEN_GEV_1.F:57-139)
 * over complex numbers: eigen_h(B) -> F = U mu^-1/2 -> C = F^H A F -> eigen_h(C) -> z = F Y.  Same argument list and
 * on-exit contract as eigx_gev: a, b, z complex(8) as interleaved (re, im) doubles, column-major, leading dimensions in
 * COMPLEX elements; upper triangles of a, b significant (Im of their diagonals ignored); w ascending; z^H B z = I; on exit
 * a holds Y, b holds F.  EIGX_ERR_NOT_SPD if B is not positive definite (message printed), EIGX_ERR_NONFINITE with
 * w = NaN for a non-finite significant entry.  Timers [0..4] as for eigx_gev.  Several ranks: a, b, z are the ranks'
 * 2-D cyclic blocks, nothing is gathered.  Inherits eigen_h's overflow above a matrix scale of about 1e77. */
int eigx_hgev(int n, double* a, int lda, double* b, int ldb, double* w, double* z, int ldz);
int eigx_hgev_dev(int n, double* a_dev, int lda, double* b_dev, int ldb, double* w_dev, double* z_dev, int ldz);

/* KMATH_EIGEN_GEV_RANGE -- EXTENSION, not in the reference: eigenpairs il .. iu of the generalised symmetric-definite
 * problem A x = lambda B x by the Cholesky route of LAPACK's dsygvd (csrc/tri.hip): B = U^T U ->
 * C = U^-T A U^-1 -> the index-range solve of C on the eigen_sx route (eigx_sx_range_dev: scaling, size rule key 17,
 * acceptance test, fallback to the full divide and conquer all stay in force) -> Z = U^-1 Y on the m columns.
 * il = 1, iu = n is a full generalised solve.  eigx_gev keeps the reference's method and on-exit contract.
 * One GPU only: with more than one rank the call prints one line and returns EIGX_ERR_BAD_ARG.
 * 1 <= il <= iu <= n, m = iu - il + 1: w(1:m) = eigenvalues il .. iu of the ascending generalised spectrum, z(:, 1:m)
 * the eigenvectors with z^T B z = I_m; nothing beyond m entries / columns of w, z is touched.  mode 'A' eigenpairs, 'N'
 * eigenvalues only (z may be NULL, no back-substitution); anything else is EIGX_ERR_BAD_ARG.  Upper triangles of a, b
 * significant (NaN in the strict lower triangles does not matter).  On exit a is destroyed and carries no statistics;
 * b holds U in its upper triangle (B = U^T U), its strict lower triangle is unspecified.  The significant triangles of
 * a AND b are scanned before anything is factored: a non-finite entry gives EIGX_ERR_NONFINITE and w(1:m) = NaN.  B not
 * positive definite: EIGX_ERR_NOT_SPD and the message of eigx_gev.  Host form: any leading dimensions.  Device form:
 * even leading dimensions, else EIGX_ERR_BAD_ARG (the rule of eigx_gev_dev); it waits on the default stream on entry.
 * eigx_get_timers [0..4] = total, factorisation, forming C, the range solve, back-substitution (the layout of eigx_gev);
 * eigx_range_info / eigx_range_timers report on the inner call.  B is NOT scaled: U carries the square root of B's
 * scale and C its inverse, so a B near either end of the fp64 range overflows or underflows there (documented, not
 * solved).  Workspace: pooled buffers named "gevr.*", one n x n matrix, panels of n x NB and the n x NB block inverses. */
int eigx_gev_range(int n, int il, int iu, double* a, int lda, double* b, int ldb, double* w, double* z, int ldz, char mode);
int eigx_gev_range_dev(int n, int il, int iu, double* a_dev, int lda, double* b_dev, int ldb, double* w_dev, double* z_dev,
                       int ldz, char mode);
/* KMATH_EIGEN_GEV_RANGE_V -- EXTENSION: the eigenpairs of A x = lambda B x with vl <= lambda < vu; eigx_gev_range with the
 * window protocol of eigx_sx_range_v (vl, vu, mmax, *m, *il, mode 'C', m = 0, EIGX_ERR_WINDOW, statuses).  B is factored and
 * C formed as in eigx_gev_range, the value window goes to the range solve of C (B is not scaled, so C's eigenvalues are the
 * generalised ones), and the back-substitution runs on the m columns found -- not at all for m = 0, modes 'N' and 'C'.
 * b holds U on exit whenever the call returns EIGX_OK; on EIGX_ERR_WINDOW the host form leaves a and b as they were
 * passed, the device form has destroyed a and holds U in b.  eigx_get_timers [0..4] as for eigx_gev_range.  The complex
 * sibling is eigx_hgev_range_v below. */
int eigx_gev_range_v(int n, double vl, double vu, int mmax, int* m, int* il, double* a, int lda, double* b, int ldb, double* w,
                     double* z, int ldz, char mode);
int eigx_gev_range_v_dev(int n, double vl, double vu, int mmax, int* m, int* il, double* a_dev, int lda, double* b_dev,
                         int ldb, double* w_dev, double* z_dev, int ldz, char mode);
/* Its stages (one GPU, device arrays, any leading dimension >= n, LAPACK uplo = 'U'; NB = eigx_tune key 20).
 * eigx_chol_dev: B = U^T U, U in place in the upper triangle, nothing below the diagonal is read; EIGX_OK, or
 * EIGX_ERR_NOT_SPD for a pivot that is not > 0 or not finite.  eigx_trsm_upper_dev: x(n, nrhs) <- op(U)^-1 x in place,
 * trans 'N' or 'T', by block inversion (the inverses of U's NB-wide diagonal blocks, then two GEMMs per block row).
 * eigx_gev_reduce_dev: upper(a) <- U^-T A U^-1 for the upper triangle of a on entry (all of a is overwritten). */
int eigx_chol_dev(int n, double* b_dev, int ldb);
int eigx_trsm_upper_dev(char trans, int n, int nrhs, const double* u_dev, int ldu, double* x_dev, int ldx);
int eigx_gev_reduce_dev(int n, double* a_dev, int lda, const double* u_dev, int ldu);

/* KMATH_EIGEN_HGEV_RANGE -- EXTENSION, not in the reference: eigenpairs il .. iu of the complex Hermitian-definite
 * problem A x = lambda B x by the Cholesky route of LAPACK's zhegvd (csrc/ztri.hip): B = U^H U ->
 * C = U^-H A U^-1 -> eigen_h of C with nvec = iu (it scales C itself) -> Z = U^-1 Y on the columns il .. iu.  The contract
 * of eigx_gev_range over complex numbers, the storage of eigx_hgev: a, b, z complex(8) as interleaved (re, im) doubles,
 * column-major, leading dimensions in COMPLEX elements.  il = 1, iu = n is a full solve at about half the cost of
 * eigx_hgev, which keeps its method and on-exit contract.
 * One GPU only: with more than one rank the call prints one line and returns EIGX_ERR_BAD_ARG.
 * 1 <= il <= iu <= n, m = iu - il + 1: w(1:m) = eigenvalues il .. iu of the ascending generalised spectrum, z(:, 1:m)
 * the eigenvectors with z^H B z = I_m; nothing beyond m entries / columns of w, z is touched.  mode 'A' eigenpairs, 'N'
 * eigenvalues only (z may be NULL, no back-substitution); anything else is EIGX_ERR_BAD_ARG.  Upper triangles of a, b
 * significant (NaN in the strict lower triangles and in Im of the diagonals does not matter).  On exit a is destroyed; b
 * holds U in its upper triangle (B = U^H U, Im of U's diagonal = 0), its strict lower triangle is unspecified.  The
 * significant triangles of a AND b are scanned before anything is factored: a non-finite entry gives EIGX_ERR_NONFINITE
 * and w(1:m) = NaN.  B not positive definite: EIGX_ERR_NOT_SPD and the message of eigx_hgev.  Host form: any leading
 * dimensions.  Device form: any leading dimensions >= n (as eigx_hgev_dev); it waits on the default stream on entry.
 * eigx_get_timers [0..4] = total, factorisation, forming C, the inner eigen_h, back-substitution.  The inner solve is
 * eigen_h, not a subset path: with il > 1 the columns 1 .. il - 1 are computed and dropped, the workspace holds an
 * n x iu complex Y, and eigx_range_info / eigx_range_timers are not written.  B is NOT scaled (the limitation of
 * eigx_gev_range).  Workspace: pooled buffers named "hgevr.*": three n x n complex matrices as split planes, C and Y
 * interleaved, panels of n x NB and the n x NB block inverses. */
int eigx_hgev_range(int n, int il, int iu, double* a, int lda, double* b, int ldb, double* w, double* z, int ldz, char mode);
int eigx_hgev_range_dev(int n, int il, int iu, double* a_dev, int lda, double* b_dev, int ldb, double* w_dev, double* z_dev,
                        int ldz, char mode);
/* KMATH_EIGEN_HGEV_RANGE_V -- EXTENSION, not in the reference: the eigenpairs of the complex problem
 * A x = lambda B x with vl <= lambda < vu; eigx_hgev_range with the window protocol of eigx_sx_range_v (vl, vu, mmax, *m,
 * *il as host pointers in both forms, mode 'C', m = 0, EIGX_ERR_WINDOW, statuses).  B is factored and C formed as in
 * eigx_hgev_range; the value window goes to eigx_h_range_v_dev on C (B is not scaled, so C's eigenvalues are the
 * generalised ones): ONE Hermitian reduction, the window's m columns of Y only, and eigx_range_info / eigx_range_timers
 * report on that inner call.  The back-substitution runs on the m columns found -- not at all for m = 0, modes 'N' and
 * 'C'.  b holds U whenever the call returns EIGX_OK; on EIGX_ERR_WINDOW the host form leaves a and b as they were passed,
 * the device form has destroyed a and holds U in b.  B not positive definite: EIGX_ERR_NOT_SPD, *m untouched.  The result
 * agrees with eigx_hgev_range on the resolved window to rounding, not bit for bit (the inner routes differ). */
int eigx_hgev_range_v(int n, double vl, double vu, int mmax, int* m, int* il, double* a, int lda, double* b, int ldb, double* w,
                      double* z, int ldz, char mode);
int eigx_hgev_range_v_dev(int n, double vl, double vu, int mmax, int* m, int* il, double* a_dev, int lda, double* b_dev,
                          int ldb, double* w_dev, double* z_dev, int ldz, char mode);
/* Its stages (one GPU, device arrays of interleaved complex(8), any leading dimension >= n in complex elements, LAPACK
 * uplo = 'U'; NB = eigx_tune key 20, shared with the real stages).
 * eigx_zchol_dev: B = U^H U, U in place in the upper triangle with a real positive diagonal (Im written as 0); nothing
 * below the diagonal and no Im of the diagonal is read; EIGX_OK, or EIGX_ERR_NOT_SPD for a pivot that is not > 0 or not
 * finite.  eigx_ztrsm_upper_dev: x(n, nrhs) <- op(U)^-1 x in place, trans 'N' or 'C' (conjugate transpose), by block
 * inversion.  eigx_hgev_reduce_dev: upper(a) <- U^-H A U^-1 for the upper triangle of a on entry (the strict lower
 * triangle of a is left as it was).  More than one rank: EIGX_ERR_INTERNAL. */
int eigx_zchol_dev(int n, double* b_dev, int ldb);
int eigx_ztrsm_upper_dev(char trans, int n, int nrhs, const double* u_dev, int ldu, double* x_dev, int ldx);
int eigx_hgev_reduce_dev(int n, double* a_dev, int lda, const double* u_dev, int ldu);

/* replaces eigen_bisect(d,e,w,n,mode) src/bisect.F:67-397 (band=1) / eigen_bisect2(d,e,f,w,n,mode)
 * src/bisect2.F:71-718 (band=2): all eigenvalues of the band matrix by Sturm counts, w_dev ascending.
 * Used by modes 'N', 'S', 'C' (alone) and 'X' (after the divide and conquer), src/eigen_sx.F:200-222. */
int eigx_band_bisect_dev(int n, const double* d_dev, const double* e_dev, int lde, int band, double* w_dev);

/* EXTENSION (no counterpart in the reference): eigenvalues il .. iu (1-based, inclusive) of the band matrix by the same
 * multi-section on an index window, w_dev[0 .. iu - il] ascending. */
int eigx_band_bisect_range_dev(int n, int il, int iu, const double* d_dev, const double* e_dev, int lde, int band,
                               double* w_dev);
/* EXTENSION: cnt_dev[p] = number of eigenvalues of the band matrix below x_dev[p], p < npts, by the Sturm count and the
 * pivmin of the multi-section (a window resolved by these counts agrees with the brackets of eigx_band_bisect_range_dev).
 * 0 for a point at or below the lower Gershgorin bound (-Inf included), n at or above the upper one (+Inf included), -1
 * for NaN.  One thread per point: npts = 2 resolves a value window, thousands give a density-of-states histogram straight
 * after a reduction.  One GPU; returns after cnt_dev is complete. */
int eigx_band_count_dev(int n, const double* d_dev, const double* e_dev, int lde, int band, int npts, const double* x_dev,
                        int* cnt_dev);
/* EXTENSION, the counterpart of eigx_band_dc_dev for a chosen set: m approximate eigenvalues w_sel_dev of the band matrix
 * (d, e(lde, 2), band 1 or 2) -> Ritz values w_out_dev[m] (ascending) and an orthonormal n x m eigenvector basis
 * z_dev(ldz, m).  One GPU.  Returns EIGX_OK, or a positive value when its acceptance test refused the result (1: a Cholesky
 * factorisation of CholQR2 broke down, 2: cond(L) above 10^key19); z_dev and w_out_dev are then not to be used. */
int eigx_band_eigvec_dev(int n, int m, const double* d_dev, const double* e_dev, int lde, int band, const double* w_sel_dev,
                         double* w_out_dev, double* z_dev, int ldz);

/* replaces eigen_common_trbakwy(n,nvec,a,lda,z,ldz,e,m,nb) src/trbakwy4.F:77-222 */
int eigx_trbak_dev(int n, int nvec, const double* a_dev, int lda, double* z_dev, int ldz,
                   const double* e_dev, int lde, int m_backward, int band);

/* replaces the BLAS dgemm call sites of the path (src/eigen_t1.F:285-295, src/trbakwy4_body.F:604-608,
 * :721-725, src/FS_PDLAED3.F90:833-860): C = alpha*op(A)*op(B)+beta*C on device arrays.
 * tri_upper != 0 restricts the update to 128x128 tiles touching the upper triangle.
 * As in BLAS, alpha == 0 or k == 0 does not reference a_dev and b_dev (C = beta*C whatever they hold, NaN and Inf
 * included), and beta == 0 does not read c_dev (it may hold NaN).  The same holds for eigx_dgemm_gather_dev, with one
 * exception: its maps are still read at index 0 when alpha == 0 or k == 0, so each map that is passed needs one readable
 * element even then. */
int eigx_dgemm_dev(char opa, char opb, int m, int n, int k, double alpha, const double* a_dev, int lda,
                   const double* b_dev, int ldb, double beta, double* c_dev, int ldc, int tri_upper);

/* same product with column gathers, as used by the D&C eigenvector update Q <- Q(:, nondeflated) * S
 * (replaces the copy into the compressed Q2 + PDGEMM of src/my_pdlaed2.F / src/my_pdlaed1.F:310-341):
 * A(:, kmap_a[k]) supplies k-index k (opa = 'N' only), B(:, kmap_b[k]) likewise (opb = 'T' only);
 * either map may be NULL.  Maps are device int arrays of length k. */
int eigx_dgemm_gather_dev(char opa, char opb, int m, int n, int k, double alpha, const double* a_dev, int lda,
                          const double* b_dev, int ldb, double beta, double* c_dev, int ldc,
                          const int* kmap_a_dev, const int* kmap_b_dev);

/* timers of the last solve, seconds: [0] total [1] reduction [2] d&c [3] back-transform [4] comm
 * (reference: TIMER_PRINT lines, src/eigen_sx.F:167-174, :300-304).  kernel-level stats for bench.py:
 * [5] trailing-update kernel seconds (sum of launches) [6] its launch count [7] its flops
 * [8] symv kernel seconds [9] its launch count [10] its algorithmic bytes */
int eigx_get_timers(double* out16);

/* Sampled in-library profiling for bench.py (the reference prints per-kernel timers under TIMER_PRINT=2,
 * src/eigen_trd.F:710-714): eigx_profile(stride>0) brackets every stride-th launch of the fused symmetric
 * mat-vec kernel and every trailing-update GEMM launch with HIP events on the library's compute stream;
 * eigx_profile_read returns {symv launches sampled, their algorithmic bytes, their seconds,
 * trailing-update launches, their flops, their seconds} accumulated since the last eigx_profile call. */
int eigx_profile(int stride);
int eigx_profile_read(double* out6);
/* the same events by kind: out[3 k + {0, 1, 2}] = {launches sampled, units, seconds} for kind k < nkinds;
 * kinds: 0 fused mat-vec, 1 trailing update, and on several ranks the rest of a sampled reduction step:
 * 2 local reduce + push of the step message (kl_kernel, or kl_kernel + the allgather in the collective form),
 * 3 wait for the peers' messages (wait kernel), 4 ka_kernel (with the wait when it is fused into it). */
int eigx_profile_read_kinds(double* out, int nkinds);

/* Tuning hook for A/B measurements (tools/, tests/): key 0 = GEMM kernel (2 = LDS-DMA ring kernel where it
 * applies [default], 1 = register-staged kernel everywhere); key 1 = target number of concurrent Sturm
 * sweeps of the bisection (default 65536); key 2 = super-block factor of the back-transformation (0 = automatic);
 * keys 3 / 4 = largest active size L that uses the 128 / 256 tile of the fused symmetric mat-vec, key 5 = active
 * size above which it streams the matrix with non-temporal loads; key 6 = 1: the trailing update streams its C tiles
 * past L2; key 7 = workgroups of the column-formation kernel beyond which a workgroup loops over row groups;
 * key 8 = chunk width (roots, 64 .. 2048) of the multi-rank D&C's eigenvector-row buffer; key 9 = doubles per slice of
 * the bounce window of the multi-rank eigenvector redistributions (keys 7-9 exist so that the tests reach the
 * large-N code paths at small sizes); key 10 = 0: the column-formation kernel always uses its largest load batches (A/B);
 * key 11 = largest active size at which the fused symmetric mat-vec uses its branch-free pipelined form; key 12 = load
 * forms of the column-formation kernel on one GPU (A/B): 2 [default] = tile scalars packed by tile index and panel dots
 * loaded once per panel column, 1 = packed tile scalars only, 0 = the earlier forms; other values are refused; keys 15 / 16 = 0:
 * the one-GPU D&C runs its passes one after the other / one product launch per merge instead of one per low height
 * (key 15 >= 2: merges larger than this use the side stream).  Index-range solves (extension): key 17 = size rule in
 * percent (0 .. 100), windows with 100 m > key17 n go straight to the full D&C; a negative value (the default, -1) selects
 * it from n by the measured table of DESIGN section 8b: 10 from n = 32768 on, 3 from n = 16384 on, 0 below (at n = 8192 the
 * subset path was slower than the nvec = m route at every m, so it is not taken there unless the key is set); key 18 = 1: eigx_sx / eigx_s / _dev calls with mode 'A' and 0 < nvec < n are routed through the range path
 * as il = 1, iu = nvec, w(nvec+1:n) filled by bisection (default 0: results bit-identical to earlier versions);
 * key 19 = log10 of the acceptance bound on cond(L) (default 6; exists so that a test can force the fallback at a small
 * size, like keys 7-9; 0 .. 16); values outside the stated ranges of keys 17 - 19 are refused.  key 20 = outer block
 * width NB of the triangular stages of eigx_gev_range (csrc/tri.hip): a multiple of 64 from 64 to 1024 (default 256), other
 * values are refused; like keys 7-9 it lets tests reach the multi-panel paths at small n.  key 21 = largest n that
 * eigx_s_batch serves with its batch kernel (0 .. EIGX_BATCH_NMAX, default EIGX_BATCH_NMAX by the measured table of DESIGN
 * section 8h; other values are refused): larger matrices go through eigx_s_dev one by one, and a test reaches that path at a
 * small n by lowering the key.  key 22 = the same for eigx_h_batch (0 .. EIGX_HBATCH_NMAX, default EIGX_HBATCH_NMAX by the
 * measured table of DESIGN section 8i; other values are refused): larger matrices go through eigx_h_dev one by one.
 * key 23 = the same for eigx_gev_batch (0 .. EIGX_GBATCH_NMAX, default EIGX_GBATCH_NMAX by the measured table of DESIGN section
 * 8j; other values are refused): larger pencils go through eigx_gev_range_dev one by one.  key 24 = the same for
 * eigx_hgev_batch (0 .. EIGX_HGBATCH_NMAX, default EIGX_HGBATCH_NMAX by the measured table of DESIGN section 8k; other values are
 * refused): larger pencils go through eigx_hgev_range_dev one by one.  key 25 = largest K at which the one-GPU trailing
 * update reads its C tile under the last MFMAs instead of before the first (0 .. 511, default 256: the measurements of
 * DESIGN sections 3 and 5; 0 = never, for A/B; other values are refused; the update is rounded as C - sum below it and as
 * -((-C) + sum) above).  key 26 = the route of eigx_s_batch_range below the cutoff of key 21, of
 * eigx_h_batch_range below that of key 22, of eigx_gev_batch_range below that of key 23 and of eigx_hgev_batch_range below that
 * of key 24: 0 = automatic (default: the
 * measured table of DESIGN section 8n, for the Hermitian family that of section 8o, for the pencils that of section 8p, for the
 * complex pencils that of section 8q), 1 = the window kernel wherever it is eligible (mode 'N', or a window no wider than
 * its n-class serves), 2 = always the full batch solve and a slice; other values are refused.  key 27 = the acceptance bound
 * of the window kernel in percent (0 .. 101, default 50: every vector keeps half its norm in the second Gram-Schmidt pass;
 * 101 refuses every matrix, so that a test reaches the redo at a small size, like key 19; other values are refused).  Returns
 * the previous value, or
 * -1 for an unknown key or a refused value.
 * Not part of the reference's interface. */
int eigx_tune(int key, int value);

/* device synchronisation helper for hosts without a HIP binding */
int eigx_device_synchronize(void);

/* device memory helpers for hosts without a HIP binding (Fortran callers, ctypes tests) */
void* eigx_malloc_dev(int64_t bytes);
int eigx_free_dev(void* p);
int eigx_memcpy_h2d(void* dst_dev, const void* src_host, int64_t bytes);
int eigx_memcpy_d2h(void* dst_host, const void* src_dev, int64_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* EIGENEXA_AMD_H */
