// eigx_context.h -- library-global state (the reference keeps the same kind of module-global state:
// TRD_COMM_WORLD, x_nnod, ... in src/eigen_devel.F:53-61; one live grid at a time, not re-entrant).
#pragma once
#include "eigx_common.h"
#include <functional>
#include <map>
#include <vector>
#include <string>
#include <type_traits>

namespace eigx {

// Workspace cache: named device buffers that persist between solves (hipMalloc of multi-GB buffers
// costs milliseconds; the reference allocates per call on the host where that is free).
// Thrown by the workspace pool when the device is out of memory; caught at the C-ABI boundary (eigx_guard), which
// tells the other ranks (their bounded waits return at once instead of running out their time limit) and returns
// EIGX_ERR_NO_MEMORY.  The reference aborts the whole job here (eigen_abort -> MPI_Abort, src/eigen_devel.F:148-164).
struct DeviceAllocError { size_t bytes; std::string name; };

struct Pool {
  struct Buf { void* p = nullptr; size_t bytes = 0; };
  std::map<std::string, Buf> bufs;
  void* get(const std::string& name, size_t bytes) {
    Buf& b = bufs[name];
    if (b.bytes < bytes) {
      if (b.p) EIGX_HIP_CHECK(hipFree(b.p));
      b.p = nullptr;
      b.bytes = 0;
      size_t want = bytes + bytes / 16 + 256;
      // EIGX_TEST_FAIL_ALLOC=<buffer name>: this allocation fails (tests of the failure path)
      static const char* fail_name = getenv("EIGX_TEST_FAIL_ALLOC");
      if ((fail_name && name == fail_name) || hipMalloc(&b.p, want) != hipSuccess) {
        (void)hipGetLastError();
        b.p = nullptr;
        throw DeviceAllocError{want, name};
      }
      b.bytes = want;
    }
    return b.p;
  }
  template <typename T> T* get_t(const std::string& name, size_t count) {
    return (T*)get(name, count * sizeof(T));
  }
  // pinned host staging buffers (one D2H / H2D copy per D&C merge step instead of sixteen pageable ones)
  std::map<std::string, Buf> hbufs;
  void* get_host(const std::string& name, size_t bytes) {
    Buf& b = hbufs[name];
    if (b.bytes < bytes) {
      if (b.p) EIGX_HIP_CHECK(hipHostFree(b.p));
      b.p = nullptr;
      size_t want = bytes + bytes / 16 + 256;
      EIGX_HIP_CHECK(hipHostMalloc(&b.p, want, hipHostMallocDefault));
      b.bytes = want;
    }
    return b.p;
  }
  void release() {
    for (auto& kv : bufs)
      if (kv.second.p) EIGX_HIP_CHECK(hipFree(kv.second.p));
    bufs.clear();
    for (auto& kv : hbufs)
      if (kv.second.p) EIGX_HIP_CHECK(hipHostFree(kv.second.p));
    hbufs.clear();
  }
};

struct CommState;  // comm.hip (peer windows + RCCL communicators for world / X / Y groups)

struct Context {
  bool initialized = false;
  int device = 0;
  Grid grid;
  hipStream_t stream = nullptr;       // compute stream
  hipStream_t side_stream = nullptr;  // collectives / copies overlapped with compute
  static constexpr int kAux = 6;
  hipStream_t aux[kAux] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // concurrent small GEMMs (D&C levels)
  hipEvent_t aux_ev[kAux + 1] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  // back-transformation plan prepared ahead (trbak_prepare_dev on the side stream during the D&C): event + key
  hipEvent_t bt_ev = nullptr;
  hipEvent_t dc_ev = nullptr;          // D&C buffers zero-filled ahead (band_dc_prepare)
  // D&C pipeline (one GPU): the secular / Loewner / eigenvector-row kernels of the NEXT pass run on dc_stream under the
  // big product of the current one; dc_b_ev = their completion, dc_z_ev = [new eigenvalues | next z] are on the host
  hipStream_t dc_stream = nullptr;
  // stream of the side work band_dc_dev runs for its caller (== side_stream; a CU-masked stream of its own changed
  // nothing: profiles/r04_bt_mask_ab.log)
  hipStream_t bt_stream = nullptr;
  hipEvent_t dc_b_ev = nullptr, dc_z_ev = nullptr;
  int dc_zero_n = 0; const double* dc_zero_qa = nullptr; const double* dc_zero_qb = nullptr;
  bool bt_ready = false;
  const double* bt_a = nullptr; double* bt_V = nullptr;
  int bt_n = 0, bt_mb = 0, bt_band = 0, bt_ldv = 0;
  Pool pool;
  CommState* comm = nullptr;
  int64_t errinfo = 0;
  double timers[16] = {0};
  // sampled HIP-event timing of the two roofline kernels (bench.py): every prof_stride-th launch of the
  // fused SYMV kernel and every trailing-update GEMM is bracketed by events on the compute stream
  int prof_stride = 0;  // 0 = off
  std::vector<hipEvent_t> prof_ev;   // pairs
  std::vector<double> prof_units;    // bytes (kind 0) or flops (kind 1) of the bracketed launch
  std::vector<int> prof_kind;
  size_t prof_used = 0;
  void prof_begin(int kind, double units, hipStream_t st) {
    if (prof_used + 2 > prof_ev.size()) {
      for (int q = 0; q < 2; ++q) { hipEvent_t e; EIGX_HIP_CHECK(hipEventCreate(&e)); prof_ev.push_back(e); }
    }
    prof_kind.push_back(kind);
    prof_units.push_back(units);
    EIGX_HIP_CHECK(hipEventRecord(prof_ev[prof_used], st));
  }
  void prof_end(hipStream_t st) {
    EIGX_HIP_CHECK(hipEventRecord(prof_ev[prof_used + 1], st));
    prof_used += 2;
  }
};

extern Context g_ctx;

void comm_report_failure(Context& ctx, const char* what);   // comm.hip: sets this rank's and every peer's sticky failure word (P > 1)

// C-ABI boundary guard of the solver entry points: a failed workspace allocation becomes an error code
template <class F>
int eigx_guard(Context& ctx, F&& f) {
  try {
    return f();
  } catch (const DeviceAllocError& e) {
    fprintf(stderr, "[eigx] out of device memory: workspace '%s' needs %zu bytes\n", e.name.c_str(), e.bytes);
    comm_report_failure(ctx, "out of device memory on this rank");
    if (hipDeviceSynchronize() != hipSuccess) (void)hipGetLastError();
    return -8;   // EIGX_ERR_NO_MEMORY
  }
}

// comm.hip
int comm_get_unique_id(void* out128);
int comm_init(Context& ctx, const void* unique_id);
void comm_free(Context& ctx);

// band_reduce.hip: A (upper triangle) -> band (d, e(:,1..band)); reflectors left in A's columns
void band_reduce_dev(Context& ctx, int n, double* A, int lda, double* d, double* e, int lde, int m, int band);

// dc.hip: zero-fill of the D&C's Q buffers on the side stream, ahead of band_dc_dev (optional)
void band_dc_prepare(Context& ctx, int n);
// dc.hip: eigen-decomposition of the band matrix (d, e(:,1..band)); w ascending, z(ldz, nvec).  side_work (the
// caller's T factors of the back-transformation) runs exactly once, when the last merge's product starts.
void band_dc_dev(Context& ctx, int n, int nvec, const double* d, const double* e, int lde, int band, double* w,
                 double* z, int ldz, const std::function<void()>& side_work = {});

// bisect.hip: eigenvalues only of the band matrix by Sturm counts (multi-section); w ascending
void band_bisect_dev(Context& ctx, int n, const double* d, const double* e, int lde, int band, double* w);

// bisect.hip: eigenvalues il .. iu (1-based, inclusive) of the ascending spectrum by the same multi-section, w[0 .. iu - il]
void band_bisect_range_dev(Context& ctx, int n, int il, int iu, const double* d, const double* e, int lde, int band,
                           double* w);

// bisect.hip (EXTENSION): cnt[p] = number of eigenvalues of the band matrix below x[p] for npts caller-given points (device
// arrays), by the Sturm count and pivmin of the multi-section; 0 at or below the lower Gershgorin bound (-Inf included), n
// at or above the upper one, -1 for NaN.  Enqueued on ctx.stream.
void band_count_dev(Context& ctx, int n, const double* d, const double* e, int lde, int band, int npts, const double* x,
                    int* cnt);

// The range solves.  range.hip holds what every family shares: range_args_ok, refuse_several_ranks, range_info_reset,
// resolve_value_window, range_window_stage and range_host_form.  The device drivers are range_solve_dev (solver.hip),
// herm_range_dev (herm.hip), gev_range_dev (gev.hip) and hgev_range_dev (hgev.hip); band_eigvec_dev, range_info and the knobs
// are subset.hip's.
// The window of a range solve.  By index: eigenpairs
// il .. iu (1-based, inclusive).  By value: those with vl <= lambda < vu, resolved into il .. iu by two Sturm counts after
// the band reduction; at most mmax of them are returned, and *m_out / *il_out (host) receive their number and the index
// of the first.  m() = the entries of w / columns of z the caller provides.
struct RangeWindow {
  bool by_value = false;
  int il = 0, iu = 0;
  double vl = 0.0, vu = 0.0;
  int mmax = 0;
  int* m_out = nullptr; int* il_out = nullptr;
  static RangeWindow index(int il_, int iu_) { RangeWindow r; r.il = il_; r.iu = iu_; return r; }
  static RangeWindow value(double vl_, double vu_, int mmax_, int* m_, int* il_) {
    RangeWindow r; r.by_value = true; r.vl = vl_; r.vu = vu_; r.mmax = mmax_; r.m_out = m_; r.il_out = il_; return r;
  }
  int m() const { return by_value ? mmax : iu - il + 1; }
};
// entries of w that a range call may write (NaN on a non-finite input), eigenvector columns it may ask room for
inline int range_w_cap(const RangeWindow& W, char mode) { return (W.by_value && mode == 'C') ? 0 : W.m(); }
inline int range_z_cap(int n, const RangeWindow& W, char mode) { const int c = range_w_cap(W, mode); return c < 1 ? 1 : (c < n ? c : n); }
// range.hip: the argument check of every range entry (mode in upper case), the refusal of a grid of several ranks
// (EIGX_ERR_BAD_ARG), and what a device driver starts from: range_info() = path 0, m (by value: 0), no cond, no seconds
bool range_args_ok(int n, const RangeWindow& W, const double* a, int lda, const double* w, const double* z, int ldz, char mode);
int refuse_several_ranks(const Context& ctx);
void range_info_reset(const RangeWindow& W);
// value window -> index window right after a reduction to the band form (d, e) = sigma times the caller's matrix: W.il,
// W.iu, *W.m_out, *W.il_out (range_window_stage)
void resolve_value_window(Context& ctx, int n, const double* d, const double* e, int lde, int band, double sigma, RangeWindow& W);
// The middle of range_solve_dev and herm_range_dev.  On entry the reduction is drained, F.t2 is set, (d, e, lde, band) is the
// band form of sigma times the matrix and W, mode (upper case) have passed range_args_ok.  Resolves a value window (W.il, W.iu
// from then on), computes w(1:m) and with mode 'A' the m band eigenvectors, keeps range_info, sets F.t3.  room(ncols) names n
// rows x ncols columns for band eigenvectors: asked for m columns on path 1, for iu on paths 2 / 3, where the n eigenvalues of
// the full D&C go to the pool buffer `wfull`.  Returns z / ld = the window's first column (paths 2 / 3: room + (il - 1) ld) and
// f_mid, the flops of the stage for finish -- or ended with the status to return at once: EIGX_ERR_WINDOW and a negative status
// of band_eigvec_dev (neither has gone through finish), a count-only or empty window (finished: EIGX_OK, w and z untouched).
struct SolveFrame;
struct RangeRoom { double* p; int ld; };
struct RangeStaged { bool ended = false; int rc = 0; double* z = nullptr; int ld = 0; double f_mid = 0.0; };
RangeStaged range_window_stage(SolveFrame& F, RangeWindow& W, char mode, const double* d, const double* e, int lde, int band,
                               double* w, const char* wfull, const std::function<RangeRoom(int)>& room);
// solver.hip (see there): the drivers of eigen_sx (band 2) / eigen_s (band 1) and of their range solve on device arrays
int solve_dev(Context& ctx, int n, int nvec, double* a, int lda, double* w, double* z, int ldz, int mf, int mb, char mode, int band, int nb);
int range_solve_dev(Context& ctx, int n, RangeWindow W, double* a, int lda, double* w, double* z, int ldz, int mf, int mb,
                    char mode, int band, bool fill_rest);

// subset.hip (EXTENSION, one GPU): eigenvectors of the band matrix for m chosen eigenvalues by inverse iteration, CholQR2
// and Rayleigh-Ritz; w_out = Ritz values (ascending), z(ldz, m) orthonormal.  EIGX_OK, or > 0: the acceptance test refused
// the result (1 Cholesky breakdown, 2 cond(L) above 10^key19); cond_out, stage_s[2] (seconds of the inverse
// iteration and of the rest) are optional.  Re-enters band_reduce_dev / band_dc_dev / trbak_dev for
// the m x m Rayleigh-Ritz problem: "red.", "dc.", "bt." buffers and a prepared back-transformation do not survive it.
int band_eigvec_dev(Context& ctx, int n, int m, const double* d, const double* e, int lde, int band, const double* w_sel,
                    double* w_out, double* z, int ldz, double* cond_out, double* stage_s);
// what the last range call did: path 1 subset, 2 fell back to the full D&C, 3 full D&C by the size rule; stage seconds
// t = {bisection, inverse iteration, orthonormalisation + Rayleigh-Ritz (or the fallback D&C), back-transformation}
struct RangeInfo { int path, m; double cond; double t[4]; };
RangeInfo& range_info();
// eigx_tune keys 17 (size rule, percent), 18 (opt-in of eigx_sx / eigx_s), 19 (log10 of the cond(L) bound)
int set_range_knob(int key, int v);
int get_range_knob(int key);
bool range_takes_subset(int n, int m);   // the size rule of key 17 (negative = automatic, see subset.hip)

// tri.hip (EXTENSION, one GPU): the triangular stages of the Cholesky-route generalised solver, upper triangles throughout.
// chol_upper_dev: B = U^T U in place (synchronous; EIGX_OK or EIGX_ERR_NOT_SPD).  tri_inverses_dev: the inverses of U's
// diagonal blocks of width nb (eigx_tune key 20) in the pool buffer gevr.inv, block K at v + K nb^2 with leading dimension
// nb; valid until the next call.  trsm_upper_dev: X(n, nrhs) <- op(U)^-1 X with them, trans 'N' or 'T'; enqueued.  upper_only (trans 'T', nrhs = n): only
// the upper triangle of the result is wanted, the rest of X is left unspecified.
struct TriInv { double* v = nullptr; int nb = 0; };
int chol_upper_dev(Context& ctx, int n, double* B, int ldb);
TriInv tri_inverses_dev(Context& ctx, int n, const double* U, int ldu);
void trsm_upper_dev(Context& ctx, char trans, int n, int nrhs, const double* U, int ldu, double* X, int ldx, const TriInv& V,
                    bool upper_only = false);
void transpose_dev(hipStream_t st, int n, const double* in, int ldi, double* out, int ldo);   // out = in^T (n x n)
int set_tri_nb(int v);
int get_tri_nb();

// zplanes.hip: complex matrices as split planes (Re and Im as two real column-major arrays of one leading dimension), shared
// by herm.hip, hgev.hip and ztri.hip.  A ZPlanes that is only read is passed like one that is written: the note behind
// each declaration names the planes the routine writes.
// zplanes: both planes of an ld x ncols matrix in ONE pool buffer `name`.  Conversions from / to interleaved complex(8)
// (leading dimensions in complex elements), enqueued; x is a local block of nr x nc, with G that of the 2-D cyclic layout:
// zexpand: the upper triangle of a -> the full Hermitian n x n matrix; zsplit: herm = the entries on or above the global
// diagonal only, Im of the diagonal := 0, w = optional scaling of column c by w[global c]^(-1/2); zjoin: upper = only the
// entries on or above the global diagonal; zconj_transpose: out = in^H (n x n).
// zgemm_planes: C = alpha op(A) B + beta C, op = none ('N') or conjugate transpose ('C'), as four real products (dgemm_dev:
// tri_mode, and the batch strides, the same for both planes of an operand).
struct ZPlanes {
  double* r = nullptr; double* i = nullptr;
  ZPlanes at(size_t off) const { return {r + off, i + off}; }   // both planes from element `off` on
};
struct ZBatch { int batch = 1; long sA = 0, sB = 0, sC = 0; int batch2 = 1; long sA2 = 0, sB2 = 0, sC2 = 0; };
ZPlanes zplanes(Context& ctx, const char* name, int ld, int ncols);
// launch grid of a kernel that strides over an nr x nc block by columns: up to 8 workgroups of 256 along a column
inline dim3 zcol_grid(int nr, int nc) { return dim3(ceil_div(nr, 256) < 8 ? ceil_div(nr, 256) : 8, nc < 65535 ? nc : 65535); }
void zexpand(hipStream_t st, const double* a, int lda, int n, const ZPlanes& P, int ld);   // writes P
void zsplit(hipStream_t st, const double* x, int ldx, int nr, int nc, bool herm, const ZPlanes& P, int ld,
            const double* w = nullptr, const Grid& G = Grid());   // writes P
void zjoin(hipStream_t st, const ZPlanes& P, int ld, int nr, int nc, bool upper, double* x, int ldx,
           const Grid& G = Grid());   // writes x, reads P
void zconj_transpose(hipStream_t st, int n, const ZPlanes& in, int ldi, const ZPlanes& out, int ldo);   // writes out
void zgemm_planes(hipStream_t st, char opA, int M, int N, int K, double alpha, const ZPlanes& A, int lda, const ZPlanes& B, int ldb,
                  double beta, const ZPlanes& C, int ldc, int tri_mode = 0, const ZBatch& zb = ZBatch());   // writes C

// ztri.hip (EXTENSION, one GPU): the complex siblings of tri.hip's stages on split planes, pool buffers "hgevr.*", the same
// outer block width (key 20).  zchol_upper_dev: B = U^H U in place, real positive diagonal, Im of B's diagonal not read and
// Im of U's written as 0 (synchronous; EIGX_OK or EIGX_ERR_NOT_SPD).  ztri_inverses_dev: the inverses of U's diagonal
// blocks, block K at v.at(K nb^2), valid until the next call.  ztrsm_upper_dev: X(n, nrhs) <- op(U)^-1 X, trans 'N' or
// 'C'; enqueued; upper_only as above (trans 'C').  hgev_reduce_dev: upper(C) = U^-H A U^-1 from the planes of the full
// Hermitian A (overwritten); enqueued.
struct ZTriInv { ZPlanes v; int nb = 0; };
int zchol_upper_dev(Context& ctx, int n, const ZPlanes& B, int ldb);   // writes B
ZTriInv ztri_inverses_dev(Context& ctx, int n, const ZPlanes& U, int ldu);   // reads U
void ztrsm_upper_dev(Context& ctx, char trans, int n, int nrhs, const ZPlanes& U, int ldu, const ZPlanes& X, int ldx,
                     const ZTriInv& V, bool upper_only = false);   // writes X
void hgev_reduce_dev(Context& ctx, int n, const ZPlanes& A, int lda, const ZPlanes& U, int ldu, const ZTriInv& V, const ZPlanes& C,
                     int ldc);   // writes A and C

// trbak.hip: T factors of the back-transformation ahead of time on stream s, and Z(:, 0:nvec) <- H_n ... H_{1+band} Z
void trbak_prepare_dev(Context& ctx, int n, double* A, int lda, const double* e, int lde, int mb, int band, hipStream_t s);
void trbak_dev(Context& ctx, int n, int nvec, double* A, int lda, double* Z, int ldz, const double* e, int lde, int mb,
               int band);

// redist.hip: eigenvector column blocks -> the callers' 2-D (block-)cyclic blocks, and a block-cyclic caller's a -> the
// cyclic layout (synchronous; EIGX_OK or EIGX_ERR_INTERNAL); one all-to-all each
void cols_to_cyclic_dev(Context& ctx, int n, int nvec, int nb, int zc, int zc0, int zcnt, const double* zcols, int ldz,
                        double* z_user, int ldz_user, hipStream_t st);
int bc_to_cyclic(Context& ctx, const double* a, int lda, int n, int nb, double* out, int ldo, hipStream_t st);
// solver.hip
int64_t solver_workspace_bytes(const Context& ctx, int n, int lda, int ldz, int mf, int mb);
// eigen_scaling of every solver (src/eigen_scaling.F:86-150): max |a| and a non-finite flag over the upper triangle of
// this rank's 2-D cyclic block of an n x n matrix (real, or interleaved complex with lda in complex elements: max of
// |Re|, |Im|, Im of the diagonal not read), combined over the ranks.  NaN / Inf anywhere: w(1:nw) = NaN (nw < 0: all n;
// an index-range solve's w may hold fewer), errinfo = -1, EIGX_ERR_NONFINITE.  Otherwise *sigma = the factor to scale
// the matrix by (1 = none; sigma == nullptr: only the scan is wanted).
int eigen_scaling(Context& ctx, const double* a, int lda, bool cplx, int n, double* w, double* sigma, int nw = -1);

// The frame of a whole solve: what eigen_sx / eigen_s (solve_dev), the index-range solves (range_solve_dev) and the two
// eigen_h drivers (herm.hip) open and close with.  A driver calls begin, (real drivers) stage_inputs, scale, marks its
// stage boundaries in t1 .. t3, and leaves through finish.  Everything is enqueued on ctx.stream in the order of the calls.
struct SolveFrame {
  Context& ctx;
  const int n;
  const bool cplx;        // eigen_h: a and z are interleaved complex, the statistics go into a(1:2,1)
  double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;   // entry; start / end of the reduction; end of the eigenvalue stage
  double sigma = 1.0;     // scale: the factor the matrix was (real) or is to be (eigen_h) scaled by
  double* a_user = nullptr;   // stage_inputs (eigen_h: herm_solve_dev): the caller's arrays behind the internal stand-ins
  double* z_user = nullptr;
  int ldz_user = 0;
  int zcols = 0;          // stage_inputs: eigenvector columns per rank of the internal z (0: the caller's z is used as it is)
  SolveFrame(Context& c, int n_, bool cplx_) : ctx(c), n(n_), cplx(cplx_) {}
  // Entry: initialised? -> n <= 0 (warning of src/eigen_sx.F:95-98) -> args_ok, the driver's own pointer and
  // leading-dimension checks -> device, the caller's default stream drained, errinfo / timers / (several ranks)
  // communication seconds reset -> t0.  EIGX_OK or the status to return.
  int begin(bool args_ok);
  // Real drivers: a (and z, if wanted) as the kernels need them -- even leading dimension, 16-byte aligned base, cyclic
  // layout (nb > 1: block-cyclic in) -- replaced by internal copies where the caller's are not.
  int stage_inputs(double*& a, int& lda, double*& z, int& ldz, bool want_vec, int nvec, int nb);
  void return_z(const double* z, int ldz, int ncols);   // one GPU: the stand-in of stage_inputs -> the caller's z
  // eigen_scaling; a non-finite input fills w(1:nw) with NaN.  Real: the upper triangle of the cyclic block is scaled by
  // sigma here; eigen_h scales where it splits the planes.
  int scale(double* a, int lda, double* w, int nw);
  // Exit: w(1:nw) /= sigma -> drain -> flops = 4/3 n^3 + f_mid + 2 bt_cols n^2 (bt_cols = 0: no back-transformation),
  // timers 0 .. 4 and 12 -> statistics into the caller's a(1:3,1) (eigen_h: a(1:2,1)) where this rank holds stat_rows > 0
  // rows of that column -> drain.  Real drivers only, as in the reference: flops negated when f_mid == 0; seconds of
  // communication in timers[4] and a(3,1) (-1 on one GPU).
  int finish(double* w, int nw, double f_mid, int bt_cols, int stat_rows);
};
// Host staging of a local block of nr x nc elements of esz (8 or 16) bytes: a pooled device buffer with the leading
// dimension host_ld(nr) (h == nullptr: allocated only), and the copy of a device block back to the host
inline int host_ld(int nr) { return pad_ld(nr + 2); }
void* host_to_dev(Context& ctx, const char* name, const void* h, int ld, int nr, int nc, int esz);
void dev_to_host(void* h, int ld, const void* d, int ldd, int nr, int nc, int esz);
// batch_frame.hip: the host frame of the batched entries, uniform, ragged and windowed.  First the pieces every
// frame is made of.
// A status that belongs to one matrix of a batch (the others are solved all the same), not to the call: out of memory, ...
bool batch_status_per_matrix(int rc);
// What every entry, host or device form, begins with: not initialised -> its status; several ranks -> refuse_several_ranks; mode
// to upper case; args_ok() (the family's predicate, which reads the mode in upper case) false -> EIGX_ERR_BAD_ARG; an empty batch
// -> EIGX_OK; hipSetDevice.  Returns true to go on, or false with the status to return in rc.
bool batch_entry_begin(Context& ctx, char& mode, int batch, const std::function<bool()>& args_ok, int& rc);
// What every device form ends with: timers[0 .. 15] = 0, then timers[0] = the seconds since t0.
void batch_entry_end(Context& ctx, double t0);
// The first-failure word of a call: a pooled unsigned long long on the device, all ones = "nothing failed"; a matrix that fails
// leaves (its index << 8 | -status) in it by atomicMin (report_failure, batch_common.h), so the lowest index wins.  arm: take the
// word from the pool and set it on `st`; dev goes to the launches; merge adds a failure found on the host (the ragged frame's
// blocks above the cutoff); finish reads the word back on `st` (not armed: nothing to read), drains `st` and, if anything
// failed, sets rc to that status and ctx.errinfo to -1 -- otherwise it leaves both alone.
// The pool name is a parameter because calls nest: route 2 of the windowed frame calls eigx_s_batch_dev, which arms batch.first
// while the outer call's word (brange.first) is live.
struct FirstFailure {
  unsigned long long* dev = nullptr;
  unsigned long long host = ~0ull;
  void arm(Context& ctx, const char* name, hipStream_t st);
  void merge(int k, int rc);
  void finish(Context& ctx, hipStream_t st, int& rc);
};
// The loop above the cutoff of a uniform batch: solve_one(k) for every matrix, its status into info[k] (device; may be null).
// Returns the first failure (or EIGX_OK), or at once a status that is not per matrix.  It does not touch ctx.errinfo.
int batch_loop_above_cutoff(int batch, int* info, const std::function<int(int)>& solve_one);
// The uniform frame (batch.hip, hbatch.hip, gbatch.hip, hgbatch.hip).  BatchArgs is a
// call: the entry's arguments, b / ldb / stride_b for a family with has_b only, and esz = bytes per element of a, b and z (8, or
// 16: interleaved complex, leading dimensions and strides in elements).  A family supplies its cutoff (n above it goes to the
// full-size solver) and two functions: launch its kernel on `st` for the n-class of g.n (with_n_class; `first` is the launch's
// first-failure word), and solve matrix k with the full-size solver (its status; g.mode is in upper case).
struct BatchArgs {
  int n, batch;
  double* a; int lda; int64_t stride_a;
  double* b; int ldb; int64_t stride_b;
  double* w; int ldw;
  double* z; int ldz; int64_t stride_z;
  char mode; int* info;
  int esz; bool has_b;
  double* block(double* p, int64_t stride, int k) const { return p + (size_t)(esz / 8) * k * stride; }   // block k of a, b or z
};
typedef void (*BatchLaunch)(const BatchArgs& g, hipStream_t st, unsigned long long* first);
typedef int (*BatchSolveOne)(Context& ctx, const BatchArgs& g, int k);
// f(std::integral_constant<int, NMAX>()) for the n-class of n: NMAX = 32, 64, 96 or 128.  TOP, the family's largest class, is
// 96 or 128: with TOP = 96 every n above 64 takes the class of 96 and the class of 128 is not instantiated.  (The classes are
// named in ascending order, which is the order of the kernel instances in the code object.)
template <int TOP, class F>
void with_n_class(int n, F&& f) {
  static_assert(TOP == 96 || TOP == 128, "the largest n-class is 96 or 128");
  if (n <= 32) return f(std::integral_constant<int, 32>());
  if (n <= 64) return f(std::integral_constant<int, 64>());
  if (TOP == 96 || n <= 96) return f(std::integral_constant<int, 96>());
  if constexpr (TOP == 128) f(std::integral_constant<int, 128>());
}
// copy (kind: any direction) of the nr x nc blocks b0 .. b0 + nb - 1 of a strided batch of elements of esz bytes, block k at
// dst + k sd / src + k ss (in elements) with leading dimensions ldd / lds; one call where both sides are evenly spaced columns
void copy_blocks(void* dst, int ldd, int64_t sd, const void* src, int lds, int64_t ss, int nr, int nc, int b0, int nb, int esz,
                 hipMemcpyKind kind);
// Host staging of a uniform batch (g: host arrays, mode in upper case; z has zcols columns and w has nw entries per matrix): a,
// b, z, w and the status words in the pool buffers `names` with the leading dimension host_ld(n), a and b copied in, dev_form on
// the staged arrays; info and w come back for every matrix, z and b for runs of consecutive matrices that succeeded.
struct BatchStageNames { const char *a, *b, *z, *w, *info; };
int batch_stage_host(Context& ctx, const BatchArgs& g, int zcols, int nw, const BatchStageNames& names,
                     const std::function<int(const BatchArgs&)>& dev_form);
// the device entry (device arrays; g.info may be null) and the host entry (host arrays) of a family
int batch_frame_dev(Context& ctx, BatchArgs g, int cutoff, BatchLaunch launch, BatchSolveOne solve_one);
int batch_frame_host(Context& ctx, BatchArgs g, int cutoff, BatchLaunch launch, BatchSolveOne solve_one);
// The windowed frame (batch_range.hip, hbatch_range.hip, gbatch_range.hip, hgbatch_range.hip; DESIGN sections 8n to 8q): eigenpairs
// il .. iu of every matrix of a BatchArgs call, w with m = iu - il + 1 entries and z with m columns per matrix.  Route 1 is the
// family's window kernel with a redo of the matrices it refused, route 2 the family's full batched solve into pooled workspace and
// a gather of the window, route 3 (n above the cutoff) the range solver of one matrix at a time; eigx_tune keys 26 and 27 and the
// record behind eigx_batch_range_info live with the frame.  A family is this record:
struct WindowFamily {
  int (*cutoff)();                                        // n above it: route 3 (the cutoff key of the family's uniform entry)
  int (*window_width)(int n);                             // the widest window route 1 serves at n in mode 'A' (0: mode 'N' only)
  bool (*route1_measured_faster)(int n, char mode, int m);   // key 26 = 0: the family's measured table
  // route 1: the window kernel on the whole call for the n-class of g.n; k0 = il - 1, accept = key 27 / 100, redo[k] = 1 marks a
  // matrix that was refused and of which nothing was written
  void (*launch)(const BatchArgs& g, int k0, int m, double accept, hipStream_t st, unsigned long long* first, int* redo);
  int (*full_solve)(const BatchArgs& c);                  // route 2: the family's eigx_*_batch_dev on a chunk (c.w, c.z, c.info: workspace)
  int (*solve_window)(Context& ctx, const BatchArgs& g, int k, int il, int iu);   // route 3: matrix k (its status; mode upper case)
  const char *first, *redo, *rw, *rz, *rinfo;             // pool names: the first-failure word, the marks, route 2's workspace
  BatchStageNames host;                                   // pool names of the host form
};
int brange_frame_dev(Context& ctx, BatchArgs g, int il, int iu, const WindowFamily& fam);
int brange_frame_host(Context& ctx, BatchArgs g, int il, int iu, const WindowFamily& fam);
// The ragged frame (vbatch.hip: eigx_s_vbatch, hvbatch.hip: eigx_h_vbatch).  VbArgs is
// a call: block k is a + off_a[k] (leading dimension lda[k]) of order n[k], its eigenvalues go to w + off_w[k], its
// eigenvectors to z + off_z[k] (ldz[k]); the six descriptor arrays are host arrays of `batch` entries, offsets and leading
// dimensions in elements of esz bytes (w: doubles).  VbDesc is what a workgroup reads of its block (k = the caller's index; its
// three offsets count doubles).
// A family supplies its cutoff, its largest n-class (top: 96 or 128) and two functions: launch its kernel of class nclass on `st`
// for `count` descriptors, one workgroup each (`first`: the call's first-failure word), and solve block k with the full-size
// solver (its status; g.mode in upper case).
struct VbDesc { int k, n, lda, ldz; int64_t off_a, off_w, off_z; };
struct VbArgs {
  int batch; const int* n;
  double* a; const int64_t* off_a; const int* lda;
  double* w; const int64_t* off_w;
  double* z; const int64_t* off_z; const int* ldz;
  char mode; int* info;
  int esz;
  // the pencil families (gvbatch.hip: eigx_gev_vbatch, hgbatch.hip: eigx_hgev_vbatch) only: has_b, and
  // the second matrix of block k at b + off_b[k] with the leading dimension ldb[k], required in both modes
  bool has_b = false;
  double* b = nullptr; const int64_t* off_b = nullptr; const int* ldb = nullptr;
  double* block(double* p, int64_t off) const { return p + (size_t)(esz / 8) * off; }   // a, b or z from element `off` on
};
// what a workgroup of a pencil family reads of its block: VbDesc with ldb and off_b (the four offsets count doubles)
struct VbPencilDesc { int k, n, lda, ldb, ldz; int64_t off_a, off_b, off_w, off_z; };
typedef void (*VbLaunch)(int nclass, int count, const VbDesc* desc, const VbArgs& g, hipStream_t st, unsigned long long* first);
typedef void (*VbPencilLaunch)(int nclass, int count, const VbPencilDesc* desc, const VbArgs& g, hipStream_t st,
                               unsigned long long* first);
typedef int (*VbSolveOne)(Context& ctx, const VbArgs& g, int k);
// the schedule of a call (eigx_vbatch_plan, pure host arithmetic): see include/eigenexa_amd_vbatch.h
int vbatch_plan(int batch, const int* n, int cutoff, int top, int* order, int* counts6);
// the device entry and the host entry of a family; the overloads with a VbPencilLaunch are those of a family with has_b
int vbatch_frame_dev(Context& ctx, VbArgs g, int cutoff, int top, VbLaunch launch, VbSolveOne solve_one);
int vbatch_frame_host(Context& ctx, VbArgs g, int cutoff, int top, VbLaunch launch, VbSolveOne solve_one);
int vbatch_frame_dev(Context& ctx, VbArgs g, int cutoff, int top, VbPencilLaunch launch, VbSolveOne solve_one);
int vbatch_frame_host(Context& ctx, VbArgs g, int cutoff, int top, VbPencilLaunch launch, VbSolveOne solve_one);
// gbatch.hip: pencil k of a uniform batch above the cutoff, through gev_range_dev (gvbatch.hip hands it its blocks)
int gbatch_solve_one(Context& ctx, const BatchArgs& g, int k);
// the same for eigenpairs il .. iu (route 3 of eigx_gev_batch_range): w(1:m) at g.w + k g.ldw, z(1:n, 1:m) at block k of g.z
int gbatch_solve_window(Context& ctx, const BatchArgs& g, int k, int il, int iu);
// Host form of a solve on a local block of nr rows: a (nc columns), b (the same; b_h == nullptr: none), z (zcols columns,
// allocated only) and w (nw entries) in the pool buffers host.a / host.b / host.z (esz 8) or host.ha / host.hb / host.hz
// (esz 16, interleaved complex) and host.w, leading dimension ldd.  What comes back, and when, is each driver's contract:
// w_back copies cnt entries of w, back ncols columns (of nrows rows, default nr) of a device block.
struct HostStage {
  const int esz, nr, ldd;
  double* a = nullptr; double* b = nullptr; double* z = nullptr; double* w = nullptr;
  HostStage(Context& c, int esz_, int nr_, int nc, const void* a_h, int lda, const void* b_h, int ldb, int zcols, int nw);
  void w_back(double* w_h, int cnt) const { if (cnt > 0) EIGX_HIP_CHECK(hipMemcpy(w_h, w, (size_t)cnt * 8, hipMemcpyDeviceToHost)); }
  void back(void* h, int ld, const double* d, int ncols, int nrows = -1) const {
    dev_to_host(h, ld, d, ldd, nrows < 0 ? nr : nrows, ncols, esz);
  }
};
// range.hip: the host form of every range entry (esz 8 or 16; has_b: the pencil families, b / ldb checked and staged).  Not
// initialised -> several ranks -> arguments; HostStage sized by range_w_cap / range_z_cap; dev_form on the staged arrays; w comes
// back on EIGX_OK or EIGX_ERR_NONFINITE (the entries written), and on EIGX_OK the m columns of z (mode 'A') and what
// rest_back copies: the statistics in a's first column, or b = U.
int range_host_form(Context& ctx, int n, const RangeWindow& W, int esz, double* a, int lda, bool has_b, double* b, int ldb, double* w,
                    double* z, int ldz, char mode, const std::function<int(const HostStage&)>& dev_form,
                    const std::function<void(const HostStage&)>& rest_back);
// gev.hip: the frame of the six generalised device drivers (gev.hip, hgev.hip).  A driver tests `initialized` and the number
// of ranks itself, then: begin (EIGX_ERR_BAD_ARG, or device set, the caller's default stream drained, t[0] taken) -> mark
// at the end of each of its first three stages -> finish (end of the last; timers[0] = total, [1 .. 4] = stages; EIGX_OK).
struct GevFrame {
  Context& ctx;
  double t[5] = {0.0, 0.0, 0.0, 0.0, 0.0}; int k = 0;
  explicit GevFrame(Context& c) : ctx(c) {}
  int begin(bool args_ok);
  void mark() { if (k < 4) t[++k] = now_s(); }
  int finish();
};
// gev.hip (EXTENSION, one GPU): the Cholesky-route range solve on device arrays (even leading dimensions); b <- U
int gev_range_dev(Context& ctx, int n, RangeWindow W, double* a, int lda, double* b, int ldb, double* w, double* z, int ldz,
                  char mode);
// B's smallest eigenvalue w(1) > 0 (read back synchronously), else report_not_spd: the message (rank 0), EIGX_ERR_NOT_SPD
bool b_is_positive_definite(const Context& ctx, const double* w);
int report_not_spd(const Context& ctx);
// Building blocks of the multi-rank KMATH_EIGEN_GEV, shared with the complex generalised solver (hgev.hip):
// z = a^T on the 2-D cyclic blocks of n x n matrices (exchange buffers in the pool as `tag`.tsend / `tag`.trecv), and the
// SUMMA panel plan: L = lcm(Px, Py), kb = the panel width (kb_want rounded up to a multiple of 2 L), kbl_x / kbl_y = its
// share per process row / column, nrp / ncp = the padded local extents.  summa_pack_a: a's columns lc0 .. lc0 + kbl_y - 1
// (out[c * nrp + r]); summa_pack_b: b's rows lr0 .. lr0 + kbl_x - 1 (out[j * kbl_x + rr]); both enqueued on st.
void dist_transpose(Context& ctx, int n, const double* a, int lda, double* z, int ldz, hipStream_t st, const char* tag = "gev");
struct SummaPlan { int L, kb, kbl_x, kbl_y, nrp, ncp; };
SummaPlan summa_plan(const Grid& G, int n, int kb_want);
void summa_pack_a(hipStream_t st, const SummaPlan& p, const double* a, int lda, int nr, int nc, int lc0, double* out);
void summa_pack_b(hipStream_t st, const SummaPlan& p, const double* b, int ldb, int nr, int nc, int lr0, double* out);

// herm.hip: eigen_h on device arrays (interleaved complex; one GPU, or this rank's 2-D cyclic blocks), and its range solve
// (EXTENSION, one GPU): modes 'A', 'N' and, by value, 'C'
int herm_solve_dev(Context& ctx, int n, int nvec, double* a, int lda, double* w, double* z, int ldz, int mf, int mb,
                   char mode);
int herm_range_dev(Context& ctx, int n, RangeWindow W, double* a, int lda, double* w, double* z, int ldz, int mf, int mb,
                   char mode);
// hgev.hip (EXTENSION, one GPU): the complex Cholesky-route range solve on device arrays (interleaved complex, every leading
// dimension >= n); b <- U
int hgev_range_dev(Context& ctx, int n, const RangeWindow& W, double* a, int lda, double* b, int ldb, double* w, double* z,
                   int ldz, char mode);

}  // namespace eigx
