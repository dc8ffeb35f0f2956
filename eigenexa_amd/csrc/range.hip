// range.hip -- what the range solves of every family share (EXTENSION, one GPU; declared in eigx_context.h): the argument
// check and the refusal of several ranks, value window -> index window, range_window_stage (the eigenvalue and band
// eigenvector stage of range_solve_dev in solver.hip and herm_range_dev in herm.hip) and range_host_form (the host entries of
// solver.hip, herm.hip, gev.hip and hgev.hip).  Host code only.
#include "eigx_context.h"
#include "../../include/eigenexa_amd.h"
#include <algorithm>
#include <cmath>

namespace eigx {

// what both entry points of the range solves require of their arguments (mode in upper case).  By value: vl < vu (a NaN
// fails it), room for at least one eigenpair unless only the count is asked for (mode 'C', value form only: w and z are
// not used), and somewhere to put m and il.
bool range_args_ok(int n, const RangeWindow& W, const double* a, int lda, const double* w, const double* z, int ldz, char mode) {
  if (n <= 0 || !a || lda < n) return false;
  if (W.by_value) {
    if (!(W.vl < W.vu) || !W.m_out || !W.il_out || (mode != 'A' && mode != 'N' && mode != 'C')) return false;
    if (mode == 'C') return true;
    if (W.mmax < 1 || !w) return false;
  } else {
    if (W.il < 1 || W.iu > n || W.il > W.iu || (mode != 'A' && mode != 'N') || !w) return false;
  }
  return mode == 'N' || (z && ldz >= n);
}
int refuse_several_ranks(const Context& ctx) {
  fprintf(stderr, "[eigx] index-range solves run on one GPU only (this grid has %d ranks)\n", ctx.grid.nranks);
  return EIGX_ERR_BAD_ARG;
}
void range_info_reset(const RangeWindow& W) {
  RangeInfo& info = range_info();
  info.path = 0; info.m = W.by_value ? 0 : W.m(); info.cond = 0.0;
  for (int q = 0; q < 4; ++q) info.t[q] = 0.0;
}

// ---- value window -> index window ------------------------------------------------------------------------------------------
// The eigenvalues with vl <= lambda < vu of the matrix whose band form (d, e) is sigma times the caller's: il = count(sigma vl)
// + 1, iu = count(sigma vu), count(x) = eigenvalues below x by band_count_dev.  The pentadiagonal count is not strictly
// monotone in floating point: iu < il - 1 is an empty window like iu = il - 1.  An infinite bound needs no count.  One
// launch, one 8-byte copy back, one stream synchronisation.
void resolve_value_window(Context& ctx, int n, const double* d, const double* e, int lde, int band, double sigma,
                          RangeWindow& W) {
  const bool lo_inf = std::isinf(W.vl), hi_inf = std::isinf(W.vu);   // vl < vu: only vl = -Inf, vu = +Inf can be
  int c[2] = {0, n};
  if (!lo_inf || !hi_inf) {
    hipStream_t st = ctx.stream;
    double* xd = ctx.pool.get_t<double>("bis.vx", 2);
    int* cd = ctx.pool.get_t<int>("bis.vcnt", 2);
    const double x[2] = {sigma * W.vl, sigma * W.vu};
    EIGX_HIP_CHECK(hipMemcpyAsync(xd, x, sizeof(x), hipMemcpyHostToDevice, st));
    band_count_dev(ctx, n, d, e, lde, band, 2, xd, cd);
    int h[2] = {0, n};
    EIGX_HIP_CHECK(hipMemcpyAsync(h, cd, sizeof(h), hipMemcpyDeviceToHost, st));
    EIGX_HIP_CHECK(hipStreamSynchronize(st));
    if (!lo_inf) c[0] = h[0];
    if (!hi_inf) c[1] = h[1];
  }
  W.il = c[0] + 1;
  W.iu = std::max(c[1], c[0]);
  *W.m_out = W.iu - W.il + 1;
  *W.il_out = W.il;
}

// ---- the window stage (see eigx_context.h) -----------------------------------------------------------------------------------
//   a value window resolved (*W.m_out, *W.il_out set): m > mmax ends the call with EIGX_ERR_WINDOW before any finish, mode 'C'
//   and m = 0 with the statistics of the reduction alone, w and z untouched -> Sturm multi-section on il .. iu -> mode 'A':
//   band_eigvec_dev (inverse iteration + CholQR2 + Rayleigh-Ritz, subset.hip) into room(m) where the size rule (eigx_tune key
//   17) allows it (path 1, no D&C workspace of the outer problem), else (path 3) and after a refusal by its acceptance test
//   (path 2) the full divide and conquer with nvec = iu into room(iu), w and the eigenvectors cut out of it.
RangeStaged range_window_stage(SolveFrame& F, RangeWindow& W, char mode, const double* d, const double* e, int lde, int band,
                               double* w, const char* wfull, const std::function<RangeRoom(int)>& room) {
  Context& ctx = F.ctx;
  const int n = F.n;
  hipStream_t st = ctx.stream;
  RangeInfo& info = range_info();
  const double t2 = F.t2;
  if (W.by_value) {
    resolve_value_window(ctx, n, d, e, lde, band, F.sigma, W);
    const int mv = *W.m_out;
    info.m = mv;
    if (mode != 'C' && mv > W.mmax) return {true, EIGX_ERR_WINDOW};
    if (mode == 'C' || mv == 0) {   // nothing to compute: the statistics of the reduction alone
      F.t3 = now_s();
      info.t[0] = F.t3 - t2;
      return {true, F.finish(w, 0, 0.0, 0, n)};
    }
  }
  RangeStaged S;
  const int il = W.il, iu = W.iu, m = iu - il + 1;
  if (mode != 'A') {
    band_bisect_range_dev(ctx, n, il, iu, d, e, lde, band, w);
    info.path = 1;
    info.t[0] = now_s() - t2;
  } else {
    int path = range_takes_subset(n, m) ? 1 : 3;
    if (path == 1) {
      double* wsel = ctx.pool.get_t<double>("sub.wsel", (size_t)m);
      band_bisect_range_dev(ctx, n, il, iu, d, e, lde, band, wsel);
      info.t[0] = now_s() - t2;
      double cond = 0.0;
      double ts[2] = {0.0, 0.0};
      const RangeRoom Z = room(m);
      const int rc_ev = band_eigvec_dev(ctx, n, m, d, e, lde, band, wsel, w, Z.p, Z.ld, &cond, ts);
      if (rc_ev < 0) return {true, rc_ev};
      info.cond = cond; info.t[1] = ts[0]; info.t[2] = ts[1];
      S.z = Z.p; S.ld = Z.ld;
      if (rc_ev > 0) path = 2;   // refused by the acceptance test
    }
    if (path != 1) {
      // the full divide and conquer for the lowest iu pairs; entries and columns il .. iu are the answer
      const double tf = now_s();
      double* wn = ctx.pool.get_t<double>(wfull, (size_t)n);
      const RangeRoom Z = room(iu);
      band_dc_dev(ctx, n, iu, d, e, lde, band, wn, Z.p, Z.ld);
      EIGX_HIP_CHECK(hipMemcpyAsync(w, wn + (il - 1), (size_t)m * 8, hipMemcpyDeviceToDevice, st));
      EIGX_HIP_CHECK(hipStreamSynchronize(st));
      info.t[2] += now_s() - tf;
      S.z = Z.p + (size_t)(il - 1) * Z.ld; S.ld = Z.ld;
    }
    info.path = path;
    S.f_mid = path == 1 ? 6.0 * (double)n * m * m : ctx.timers[11];
  }
  F.t3 = now_s();
  return S;
}

// ---- the host form (see eigx_context.h) --------------------------------------------------------------------------------------
int range_host_form(Context& ctx, int n, const RangeWindow& W, int esz, double* a, int lda, bool has_b, double* b, int ldb, double* w,
                    double* z, int ldz, char mode, const std::function<int(const HostStage&)>& dev_form,
                    const std::function<void(const HostStage&)>& rest_back) {
  if (!ctx.initialized) return EIGX_ERR_NOT_INITIALIZED;
  if (ctx.grid.nranks != 1) return refuse_several_ranks(ctx);
  mode = upper_case(mode);
  if (!range_args_ok(n, W, a, lda, w, z, ldz, mode) || (has_b && (!b || ldb < n))) return EIGX_ERR_BAD_ARG;
  const int wcap = range_w_cap(W, mode);
  const HostStage S(ctx, esz, n, n, a, lda, has_b ? b : nullptr, ldb, mode == 'A' ? range_z_cap(n, W, mode) : 1, std::max(wcap, 1));
  const int rc = dev_form(S);
  const int m = (W.by_value && rc == EIGX_OK) ? (mode == 'C' ? 0 : *W.m_out) : wcap;   // entries that were written
  if (rc == EIGX_OK || rc == EIGX_ERR_NONFINITE) S.w_back(w, m);
  if (rc != EIGX_OK) return rc;   // (EIGX_ERR_WINDOW: a and b are as the caller passed them, ready for the retry by index)
  if (mode == 'A') S.back(z, ldz, S.z, m);   // (m = 0: nothing)
  rest_back(S);
  return EIGX_OK;
}

}  // namespace eigx
