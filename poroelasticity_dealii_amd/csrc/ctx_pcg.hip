// Krylov drivers on one system description (KrylovSystem, ctx_internal.hpp): device-controlled PCG (SolverCG restated), its single-reduction form for partitioned runs, the host-driven form for SSOR / ILU(0); the lambda_max estimate.
#include <dlfcn.h>
#include <rccl/rccl.h>
#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <thread>
#include <unordered_map>
#include "common.hpp"
#include "ctx_internal.hpp"

using namespace poro;
using namespace poro::ctx_detail;

namespace poro {
namespace ctx_detail {
// Expected iteration count of a solve from the counts of the last two solves of the system (a transient's warm-started counts drift steadily): their linear extrapolation, not
// below half the last count.  It must not run away after an atypical solve (a warm restart that took 3 iterations, followed by a real step): never more than a quarter above the
// last count, and nothing above it where an overshoot is expensive.  0: no history
static int expected_iterations(const int *hint, bool cheap_overshoot) {
  if (!hint || hint[0] <= 0) return 0;
  const int expect = std::max(hint[1] > 0 ? 2 * hint[0] - hint[1] : hint[0], hint[0] / 2);
  return std::min(expect, cheap_overshoot ? hint[0] + std::max(2, hint[0] / 4) : hint[0]);
}
// what both device-controlled drivers report; `own`: the operator applications of the driver's recurrence.  A preconditioner that applies the operator itself reports the useful
// ones on either driver: one per iteration + the initial residual, and prec.applications per call (one call per iteration + the first direction)
template <class State> static int finish_solve(const KrylovSystem &sys, const State &hs, int64_t own, double seconds, poro_solve_info *info) {
  if (sys.hint) { sys.hint[1] = sys.hint[0]; sys.hint[0] = hs.it; }
  if (info) { info->iterations = hs.it; info->converged = hs.converged; info->initial_residual = hs.res0; info->final_residual = hs.res; info->seconds = seconds;
              info->operator_applications = sys.prec.applications ? (int64_t)(1 + sys.prec.applications) * (hs.it + 1) : own; }
  return hs.converged ? 0 : 1;
}

// ---- single-reduction PCG for partitioned runs (Chronopoulos & Gear) ------------------------------------------------------------------
// Same Krylov space, same stopping test and same iteration count as SolverCG's recurrence in exact arithmetic, rearranged so that an iteration
// costs ONE all-reduce: z = P^-1 g, w = A z, then {g.z, w.z, g.g} in one reduction, then d = -z + beta d, s = -w + beta s (= A d), x += alpha d,
// g += alpha s.  Per iteration: 1 operator application (1 grouped neighbour exchange) + the exchanges inside P^-1 + 1 all-reduce of 4 doubles.
// The price is two more vector passes than pcg(), which is why single-rank runs keep the three-kernel recurrence.  Nothing here is gated (sys.h serves as s)
static int pcg_single_reduction(poro_ctx *c, const KrylovSystem &sys, const poro_solver_opts *opts, poro_solve_info *info) {
  hipStream_t s = c->stream;
  const int64_t n = sys.n, n_own = owned(c, n, sys.plane);
  DevBuf<double> &wbuf = c->cg1_w[sys.cg1_set], &zbuf = c->cg1_z[sys.cg1_set];
  if (wbuf.n < (size_t)n) { wbuf.alloc(n); zbuf.alloc(n); }
  if (!c->cg1_state.p) c->cg1_state.alloc(1);
  const PrecFn &precond = sys.prec.fn;
  double *x = sys.x, *g = sys.g, *d = sys.d, *sv = sys.h, *w = wbuf.p, *z = precond ? sys.prec.z : zbuf.p;
  if (!z) throw Error("pcg: explicit preconditioner without a z vector");
  const bool jacobi = opts->preconditioner == PORO_PREC_JACOBI;
  Cg1State *st = c->cg1_state.p; double *part = c->partials.p, *red = c->red.p;
  EventPair ev(c); PORO_HIP(hipEventRecord(ev.e0, s));
  sys.apply(x, w, nullptr);
  pcg_init_residual(s, g, w, sys.b, sys.inert, n);        // g = A x - b, zero on the inert dofs
  la_fill(s, d, 0.0, n); la_fill(s, sv, 0.0, n);
  double *z1_out = sys.z1.out; double z1_scale = sys.z1.scale;
  if (jacobi && !precond) { z1_out = z; z1_scale = 1.0; }   // Jacobi: the update kernel also leaves z = D^-1 g_new for the next iteration (in place of z)
  Cg1State hs{};
  int enq = 0;
  const int expect = expected_iterations(sys.hint, false);
  auto next_batch = [&](int done_its) { const int left = expect - 4 - done_its; return left >= 4 ? std::min(32, left) : 2; };
  int batch = expect > 0 ? next_batch(0) : 1;
  while (true) {
    for (int k = 0; k < batch; ++k) {
      if (precond) { PrecCall call; call.z1_ready = enq > 0 && sys.z1.out != nullptr; (void)precond(g, z, call); }      // (stored by the previous cg1_update)
      else if (jacobi) { if (enq == 0) la_cheb_first(s, z, g, sys.diag, 1.0, n); }   // z = D^-1 g (zero on the inert dofs); after the first iteration the update kernel stores it with the new residual
      else la_copy(s, z, g, n);
      sys.apply(z, w, nullptr);
      cg1_dots(s, g, z, w, enq == 0 ? sys.b : nullptr, n_own, part);
      pcg_scalars_sum(s, part, 4, red);
      allreduce_sum(c, red, 4);
      cg1_scalars(s, st, red, enq == 0 ? 1 : 0, opts->abs_tol, opts->rel_tol, opts->max_iter, opts->stop_rule);
      cg1_update(s, st, d, sv, x, g, z, w, sys.diag, sys.inert, z1_out, z1_scale, n);
      ++enq;
    }
    PORO_HIP(hipMemcpyAsync(&hs, st, sizeof(hs), hipMemcpyDeviceToHost, s)); PORO_HIP(hipStreamSynchronize(s));
    if (hs.done) break;
    // (the preconditioner and operator launches of an iteration are not gated by the device-side `done` flag: without a hint poll at least every 8 iterations)
    if (expect > 0) batch = next_batch(enq); else if (batch < 8) batch *= 2;
  }
  PORO_HIP(hipEventRecord(ev.e1, s)); PORO_HIP(hipEventSynchronize(ev.e1));
  float ms = 0; PORO_HIP(hipEventElapsedTime(&ms, ev.e0, ev.e1));
  return finish_solve(sys, hs, hs.it + 2, ms * 1e-3, info);   // initial residual + one per iteration + the one that found the converged residual
}

// ---- PCG with device-side control: SolverCG<>::solve restated, Jacobi instead of SSOR ---------------
// The system, its operator and its preconditioner: KrylovSystem, ApplyFn and PrecFn / PrecCall in ctx_internal.hpp.  The vector kernels compute alpha / beta / the stopping test in
// their prologues: from the block partials (single rank, 3 launches per iteration incl. the operator) or from the all-reduced scalars (partitioned).  An explicit preconditioner
// writes z between the two update kernels; the scalars stay on the device exactly as in the Jacobi case.  Its FIRST call of a solve is ungated and asked for no g . z (the
// first-direction kernel computes it); every later one gets PrecCall{gate (if prec.gated), gz_partials, z1_ready (if z1.out)}.
int pcg(poro_ctx *c, const KrylovSystem &sys, const poro_solver_opts *opts, poro_solve_info *info) {
  static const bool two_reductions = std::getenv("PORO_TWO_REDUCTION_CG") != nullptr;    // A/B hook: the three-kernel recurrence on partitioned runs too
  const FdmOct *oct = sys.oct.form;
  const bool multi = c->comm.multi();
  if (multi && !two_reductions && !oct) return pcg_single_reduction(c, sys, opts, info);
  hipStream_t s = c->stream;
  const PrecFn &precond = sys.prec.fn;
  const int prec = opts->preconditioner == PORO_PREC_JACOBI ? 1 : 0;
  if (oct && (!precond || multi != oct->slab.on)) throw Error("pcg: the octant form needs an explicit preconditioner (one rank: octants, slab partition: quadrants)");
  const int64_t n = sys.n, n_own = owned(c, n, sys.plane);
  double *x = sys.x, *d = sys.d, *h = sys.h, *g = oct ? oct->g.p : sys.g, *zbuf = oct ? oct->z.p : sys.prec.z;
  if (precond && !zbuf) throw Error("pcg: explicit preconditioner without a z vector");
  double *part = c->partials.p, *red = c->red.p; PcgScalars *sc = c->scal.p;
  double *part_dh = part + 3 * (size_t)kMaxPartials;      // slots of the fused / separate d.h partials
  const auto t_start = std::chrono::steady_clock::now();
  // g = A x - b ; d = -P^-1 g ; gh = g.P^-1 g
  sys.apply(x, h, nullptr);
  if (oct) fdmo_init_residual(s, *oct, g, h, sys.b, sys.inert); else pcg_init_residual(s, g, h, sys.b, sys.inert, n);
  if (opts->stop_rule != PORO_STOP_REDUCTION) la_dot_partials(s, sys.b, sys.b, n_own, part);     // ||b||^2 only enters the ||b||-relative stopping rule (the slot keeps an older, finite value otherwise)
  if (precond) (void)precond(g, zbuf, PrecCall{});
  if (oct) fdmo_first_direction(s, *oct, d, g, zbuf, part + kMaxPartials); else pcg_first_direction(s, d, g, sys.diag, zbuf, prec, n, n_own, part + kMaxPartials);
  pcg_scalars_sum(s, part, 3, red);
  allreduce_sum(c, red, 3);
  pcg_scalars_start(s, sc, red, opts->abs_tol, opts->rel_tol, opts->max_iter, opts->stop_rule);
  PORO_HIP(hipMemsetAsync(part_dh, 0, kMaxPartials * sizeof(double), s));
  PcgScalars hs{};
  int it = 0;
  // Iterations are enqueued in batches, THEN the device-side state is polled (a host round trip idles the GPU for ~50 us).  Launches behind the finishing
  // iteration are no-ops (the vector kernels, the structured operator and the fused Chebyshev kernels test the device-side flag; ~1 us each), so where
  // everything is gated an overshoot is cheaper than a poll; an ungated explicit preconditioner (fast diagonalisation) is not, so its batches stop short.
  const bool cheap_overshoot = !precond || sys.prec.gated;
  const int expect = expected_iterations(sys.hint, cheap_overshoot);
  const bool small = n <= 400000;     // launch-bound sizes: an ungated preconditioner application costs less than the idle time of a poll
  int batch = expect > 0 ? (cheap_overshoot ? std::min(expect, 256) : std::max(1, expect - 1)) : (precond && !cheap_overshoot && !small ? 1 : 4);   // no history: a poll (~15 us through the mailbox) every 4 iterations
  PrecCall call;
  call.gate = sys.prec.gated ? sc : nullptr; call.gz_partials = part + kMaxPartials; call.z1_ready = sys.z1.out != nullptr;
  // A gated preconditioner on one rank that can (prec.decides_stop): the stopping test of an iteration runs in the first kernel of its preconditioner call, on the g . g partials the
  // residual update has just stored, and the finishing iteration skips the whole call - its z would never be read.  The direction update then takes the stored decision.
  // PORO_PCG_FINAL_PREC (A/B hook, read once per solve): the test behind the preconditioner, in the direction update, as everywhere else
  const bool stop_in_prec = oct && !multi && sys.prec.gated && sys.prec.decides_stop && std::getenv("PORO_PCG_FINAL_PREC") == nullptr;
  // Two more A/B hooks, read once per solve, both restoring what was there before: PORO_PCG_STOP_PER_WAVE - every wave of the transform pass adds up all the g . g partials for
  // itself (four-wave workgroups share the sum out otherwise); PORO_PCG_GG_RESUM - the direction update adds them up once more instead of reading the sum the test stored
  const int stop_per_wave = std::getenv("PORO_PCG_STOP_PER_WAVE") != nullptr ? 1 : 0;
  const bool gg_stored = stop_in_prec && std::getenv("PORO_PCG_GG_RESUM") == nullptr;
  while (true) {
    for (int k = 0; k < batch; ++k) {
      ++it;
      if (stop_in_prec) call.stop = PcgStopTest{sc, part, it, stop_per_wave};
      // operator (+ fused or separate d.h partials).  A fused dot runs over ALL local rows of the pre-exchange partial product, which
      // sums to the global d.Ad over the ranks; the separate kernel sees the exchanged h and therefore skips the upper shared plane.
      if (!sys.apply(d, h, part_dh)) pcg_dot_dh(s, sc, d, h, n_own, part_dh);
      if (multi) { pcg_scalars_sum(s, part_dh, 1, red); allreduce_sum(c, red, 1); }
      if (oct) fdmo_update_g(s, *oct, sc, (it - 1) & 1, g, h, sys.inert, part_dh, part, multi ? red : nullptr);
      else pcg_update_g_fused(s, sc, (it - 1) & 1, g, h, sys.diag, zbuf, sys.z1.out, sys.z1.scale, prec, n, n_own, part_dh, multi ? red : nullptr, part);
      const GzLeft gz = precond ? precond(g, zbuf, call) : GzLeft::in_partials;     // (Jacobi / none: the residual update has left g . z)
      if (gz == GzLeft::nowhere) {
        if (oct && multi) fdmo_dot_owned(s, *oct, g, zbuf, call.gz_partials, call.gate);
        else la_dot_partials(s, g, zbuf, oct ? oct->n_oct : n_own, call.gz_partials, call.gate);
      }
      if (multi) { pcg_scalars_sum(s, part, 2, red + 1); allreduce_sum(c, red + 1, 2); }
      // (octant form: the transform passes leave their g . z partials in oct->gz_part - one per workgroup of pass 2, more than kMaxPartials - not in `part`)
      if (oct) fdmo_update_d(s, *oct, sc, (it - 1) & 1, it, x, d, zbuf, part, multi ? red + 1 : nullptr, gz == GzLeft::in_octant_form, sys.oct.stream_x, stop_in_prec, gg_stored);
      else pcg_update_d_fused(s, sc, (it - 1) & 1, it, x, d, g, sys.diag, zbuf, prec, n, part, multi ? red + 1 : nullptr);
    }
    post_and_wait(c, nullptr, 0, sc); hs = c->mailbox->sc;
    if (hs.done || hs.finishing) break;
    if (expect > 0) batch = cheap_overshoot ? 3 : small ? 2 : 1;
    else if (cheap_overshoot && precond) batch = 4;          // (an explicit preconditioner: a no-op iteration still costs ~8 launches)
    else if (batch < 32) batch *= 2;
  }
  // (the last poll returned after the finishing iteration: the solve is complete on the device; wall time of the solve on the host clock.  Operator applications: the initial
  // residual + one per iteration; launches enqueued behind the finishing iteration are no-ops and are not counted)
  if (hs.stop) c->timers["fdm_u_final_prec_skipped"].enqueued++;      // (a count, no time: the solves whose finishing iteration skipped its preconditioner call)
  return finish_solve(sys, hs, hs.it + 1, std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count(), info);
}

// ---- PreconditionSSOR fidelity mode: SolverCG with the reference's SSOR(omega) in natural row order ---------------------------
void build_ssor_levels(poro_ctx *c, CsrDev &A) {
  if (A.ssor.built) return;
  std::vector<int64_t> rp(A.n + 1); std::vector<int32_t> col(A.nnz);
  PORO_HIP(hipMemcpy(rp.data(), A.rp.p, (A.n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost)); PORO_HIP(hipMemcpy(col.data(), A.col.p, A.nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
  auto levels = [&](bool fwd, DevBuf<int32_t> &rows_dev, std::vector<int64_t> &off) {
    std::vector<int32_t> lvl(A.n, 0); int maxl = 0;
    if (fwd) for (int64_t r = 0; r < A.n; ++r) { int l = 0; for (int64_t j = rp[r]; j < rp[r + 1] && col[j] < r; ++j) l = std::max(l, lvl[col[j]] + 1); lvl[r] = l; maxl = std::max(maxl, l); }
    else for (int64_t r = A.n - 1; r >= 0; --r) { int l = 0; for (int64_t j = rp[r + 1] - 1; j >= rp[r] && col[j] > r; --j) l = std::max(l, lvl[col[j]] + 1); lvl[r] = l; maxl = std::max(maxl, l); }
    off.assign(maxl + 2, 0);
    for (int64_t r = 0; r < A.n; ++r) off[lvl[r] + 1]++;
    for (int l = 0; l <= maxl; ++l) off[l + 1] += off[l];
    std::vector<int32_t> rows(A.n); std::vector<int64_t> pos(off.begin(), off.end() - 1);
    for (int64_t r = 0; r < A.n; ++r) rows[pos[lvl[r]]++] = (int32_t)r;
    rows_dev.upload(rows);
  };
  levels(true, A.ssor.fwd_rows, A.ssor.fwd_off); levels(false, A.ssor.bwd_rows, A.ssor.bwd_off);
  A.ssor.built = true;
}
// global dot product on the host; n = rows this rank owns (the upper shared plane belongs to the neighbour)
double dot_host(poro_ctx *c, const double *a, const double *b, int64_t n) {
  la_dot_partials(c->stream, a, b, n, c->partials.p); la_reduce_finish(c->stream, c->partials.p, 1, c->red.p, 0);
  allreduce_sum(c, c->red.p, 1);
  post_and_wait(c, c->red.p, 1);
  return c->mailbox->vals[0];
}
// SolverCG<>::solve with an explicit preconditioner z = P^-1 g (sys.prec.fn, called with an empty PrecCall; z lands in sys.h), host-driven scalars.  Used where an application
// of P^-1 is many launches anyway (SSOR / ILU(0) sweeps); one rank, so every row is owned
static int pcg_host(poro_ctx *c, const KrylovSystem &sys, const poro_solver_opts *opts, poro_solve_info *info) {
  hipStream_t s = c->stream;
  const int64_t n = sys.n, n_own = n;
  double *x = sys.x, *g = sys.g, *d = sys.d, *h = sys.h; const double *b = sys.b;
  const auto t0 = std::chrono::steady_clock::now();
  int64_t applies = 0; int it = 0, conv = 0;
  sys.apply(x, g, nullptr); ++applies;
  la_axpy(s, g, -1.0, b, n);                                     // g = A x - b
  double res = std::sqrt(dot_host(c, g, g, n_own)); const double res0 = res;
  const double tol = std::max(opts->abs_tol, opts->rel_tol * (opts->stop_rule == PORO_STOP_REDUCTION ? res0 : std::sqrt(dot_host(c, b, b, n_own))));
  if (res <= tol) conv = 1;
  else {
    (void)sys.prec.fn(g, h, PrecCall{});
    la_fill(s, d, 0.0, n); la_axpy(s, d, -1.0, h, n);          // d = -h
    double gh = dot_host(c, g, h, n_own);
    while (true) {
      ++it;
      sys.apply(d, h, nullptr); ++applies;
      const double alpha = gh / dot_host(c, d, h, n_own);
      la_axpy(s, g, alpha, h, n); la_axpy(s, x, alpha, d, n);
      res = std::sqrt(dot_host(c, g, g, n_own));
      if (res <= tol) { conv = 1; break; }
      if (it >= opts->max_iter) break;
      (void)sys.prec.fn(g, h, PrecCall{});
      const double beta_old = gh; gh = dot_host(c, g, h, n_own);
      la_xpby(s, d, gh / beta_old, -1.0, h, n);                   // d = beta d - h
    }
  }
  PORO_HIP(hipStreamSynchronize(s));
  if (info) { info->iterations = it; info->converged = conv; info->initial_residual = res0; info->final_residual = res; info->operator_applications = applies;
              info->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
  return conv ? 0 : 1;
}

// ---- ILU(0): factorisation and solves on the device, both level-scheduled in the natural row order (la_ilu0_factor, la_ilu_apply) -----------------
void ilu0_factor(poro_ctx *c, const CsrDev &A, const double *val, DevBuf<double> &lu_dev) {
  std::vector<int64_t> rp(A.n + 1);
  PORO_HIP(hipMemcpy(rp.data(), A.rp.p, (A.n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
  int64_t longest = 0; for (int64_t i = 0; i < A.n; ++i) longest = std::max(longest, rp[i + 1] - rp[i]);
  if (longest > 512) throw Error("ILU(0): rows longer than 512 entries are not supported by the device factorisation");
  if (lu_dev.n < (size_t)A.nnz) lu_dev.alloc(A.nnz);
  DevBuf<int> flag; flag.alloc(1); flag.zero(c->stream);
  PORO_HIP(hipMemcpyAsync(lu_dev.p, val, A.nnz * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  la_ilu0_factor(c->stream, A, A.ssor, lu_dev.p, flag.p);
  int h = 0; PORO_HIP(hipMemcpyAsync(&h, flag.p, sizeof(int), hipMemcpyDeviceToHost, c->stream)); PORO_HIP(hipStreamSynchronize(c->stream));
  if (h) throw Error("ILU(0): zero pivot in row " + std::to_string(h - 1));
}
// PreconditionSSOR(omega) / ILU(0) in the natural row order: single-rank fidelity modes, both level-scheduled on the device
int pcg_csr_sweeps(poro_ctx *c, CsrDev &A, const double *val, DevBuf<double> &lu, bool &lu_valid, KrylovSystem &sys, const poro_solver_opts *opts, poro_solve_info *info) {
  const bool ilu = opts->preconditioner == PORO_PREC_ILU0;
  if (c->comm.multi()) throw Error(ilu ? "PORO_PREC_ILU0 is implemented for one rank (the factorisation is sequential in the row order)" : "PORO_PREC_SSOR is a single-rank fidelity mode (the sweeps are order dependent)");
  build_ssor_levels(c, A);
  if (ilu && !lu_valid) { ilu0_factor(c, A, val, lu); lu_valid = true; }
  const double om = opts->omega > 0 ? opts->omega : 1.0;
  sys.n = A.n;
  sys.apply = [&, val](const double *v, double *y, double *) { la_csr_spmv(c->stream, A, val, v, y); return false; };
  sys.prec.fn = [&, val, ilu, om](const double *g, double *z, const PrecCall &) {
    if (ilu) la_ilu_apply(c->stream, A, lu.p, A.ssor, g, z); else la_ssor_apply(c->stream, A, val, A.ssor, om, g, z);
    return GzLeft::nowhere;
  };
  return pcg_host(c, sys, opts, info);
}

// lambda_max(D^-1 A_u) from the Lanczos tridiagonal of 25 Jacobi-preconditioned CG steps on a synthetic right-hand side (the constrained rows are
// inert): the largest Ritz value approaches lambda_max from below within a fraction of a percent, far faster than a power iteration
double estimate_lmax_u(poro_ctx *c, const KrylovSystem &sys) {
  const ApplyFn &apply = sys.apply; const DiagVec &dj = sys.diag; const uint8_t *inert = sys.inert;
  hipStream_t s = c->stream; const int64_t n = c->n_u, n_own = owned(c, n, c->comm.part.plane_u);
  std::vector<double> hv(n); for (int64_t i = 0; i < n; ++i) hv[i] = std::sin(0.731 * (double)i) + 0.3 * std::cos(0.013 * (double)i * (double)(i % 7));
  DevBuf<double> r, z, p, ap; r.upload(hv); z.alloc(n); p.alloc(n); ap.alloc(n);
  exchange_add(c, r.p, n, c->comm.part.plane_u);                      // partitioned runs: the start vector was filled by LOCAL index - make the copies of the shared dofs agree (any consistent vector will do)
  la_mask_zero(s, r.p, inert, n);
  la_cheb_first(s, z.p, r.p, dj, 1.0, n);                            // z = D^-1 r
  la_copy(s, p.p, z.p, n);
  double rz = dot_host(c, r.p, z.p, n_own);
  const int K = 25; std::vector<double> al, be;
  for (int k = 0; k < K && rz > 0; ++k) {
    apply(p.p, ap.p, nullptr);
    la_mask_zero(s, ap.p, inert, n);
    const double pap = dot_host(c, p.p, ap.p, n_own);
    if (!(pap > 0)) break;
    const double alpha = rz / pap;
    la_axpy(s, r.p, -alpha, ap.p, n);
    la_cheb_first(s, z.p, r.p, dj, 1.0, n);
    const double rz_new = dot_host(c, r.p, z.p, n_own), beta = rz_new / rz;
    al.push_back(alpha); be.push_back(beta);
    la_xpby(s, p.p, beta, 1.0, z.p, n);                               // p = beta p + z
    rz = rz_new;
  }
  const int m = (int)al.size();
  if (m == 0) return 4.0;
  std::vector<double> T((size_t)m * m, 0.0);
  for (int k = 0; k < m; ++k) {
    T[(size_t)k * m + k] = 1.0 / al[k] + (k > 0 ? be[k - 1] / al[k - 1] : 0.0);
    if (k + 1 < m) T[(size_t)k * m + k + 1] = T[(size_t)(k + 1) * m + k] = std::sqrt(be[k]) / al[k];
  }
  return 1.05 * sym_lambda_max(m, T);
}

}  // namespace ctx_detail
}  // namespace poro
