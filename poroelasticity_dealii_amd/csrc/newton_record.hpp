// Host-only: the record of the pressure Newton loop's gated batches (ctx_pressure.hip: poro_pres_newton_loop) and what the host rebuilds from it.  Free of HIP and of project
// headers: the library plans its batches and reads their records with these functions, and tests/newton_record_check.cpp runs them under the sanitizers.
//
// A batch is a run of up to kNewtonSlots pressure iterations enqueued without a wait.  Slot j holds the two parts of one iteration of PoroelasticityFSS.h:358-380:
//   residual part: update_volumetric_strain, assemble_residual, the test l2 < pressure_tol (closes the gate: converged)
//   solve part:    the direct solve, its check against the reference's stopping rule (closes the gate: fallback), p += dp
// Only slot 0 may come without its residual part (an iteration whose residual an earlier batch evaluated) and only the last slot without its solve part (the iteration
// at which the loop is expected to converge).  The device writes, per batch, rec[kNewtonRecord]:
//   rec[0] residual parts that ran   rec[1] solve parts whose check held   rec[2] the code: 0 gate open, 1 converged, 2 fallback   rec[3] max |p| behind the batch
//   rec[kNewtonHead + 3 j + 0] R . R of slot j   + 1, + 2: |J dp - R|^2 and |R|^2 of slot j's check
#pragma once
#include <cmath>
#include <vector>

namespace poro {

constexpr int kNewtonSlots = 4, kNewtonHead = 4, kNewtonRecord = kNewtonHead + 3 * kNewtonSlots;   // 16 doubles: the mailbox's payload
constexpr int kNewtonDefaultResiduals = kNewtonSlots;   // without a prediction: as many iterations as one batch holds (launches behind a closed gate cost a few microseconds, a second batch a wait)
enum NewtonCode { kNewtonOpen = 0, kNewtonConverged = 1, kNewtonFallback = 2 };

struct NewtonBatch { int slots = 0; bool first_residual = true, last_solve = true; };

// What the per-call loop would have produced so far.  entered = pressure_iteration; l2[i] the residual norm of iteration i + 1; res / bn the check of every solve part that
// ran (the failed one of a fallback included, which is then the last entry and is NOT counted in solves)
struct NewtonState {
  int entered = 0, solves = 0;
  bool solve_pending = false;   // iteration `entered` has its residual (not converged) and waits for its solve part
  bool finished = false; int code = kNewtonOpen;
  double pinf = 0;
  std::vector<double> l2, res, bn;
};

// The next batch.  predicted: the number of residual evaluations the same call took in the previous step (0: unknown)
inline NewtonBatch newton_plan_batch(const NewtonState &S, int max_iterations, int predicted) {
  NewtonBatch B;
  if (S.finished) return B;
  const int want = predicted > 0 ? predicted : kNewtonDefaultResiduals;
  int room = kNewtonSlots;
  if (S.solve_pending) { B.slots = 1; B.first_residual = false; --room; }
  const int remaining = max_iterations - S.entered;
  int fresh = S.entered < want ? want - S.entered : 2;      // past the prediction: two whole iterations at a time
  if (fresh > remaining) fresh = remaining;
  if (fresh > room) fresh = room;
  if (fresh < 0) fresh = 0;
  B.slots += fresh;
  // the iteration at which convergence is expected is enqueued without its solve part - unless it is the last one the cap allows, whose solve the loop always runs
  const int last = S.entered + fresh;
  B.last_solve = fresh == 0 || last != want || last == max_iterations;
  return B;
}

// Walks the slots of batch B against its record and appends what ran to S.  Returns false where the record contradicts the batch (S is then unusable)
inline bool newton_absorb(NewtonState &S, const NewtonBatch &B, const double *rec, int max_iterations) {
  if (S.finished || B.slots < 1 || B.slots > kNewtonSlots) return false;
  const int n_res = (int)rec[0], n_ok = (int)rec[1], code = (int)rec[2];
  if ((double)n_res != rec[0] || (double)n_ok != rec[1] || (double)code != rec[2] || code < kNewtonOpen || code > kNewtonFallback) return false;
  int seen_res = 0, seen_ok = 0; bool closed = false;
  if (!B.first_residual && !S.solve_pending) return false;
  if (B.first_residual && S.solve_pending) return false;
  for (int j = 0; j < B.slots && !closed; ++j) {
    const bool has_residual = j > 0 || B.first_residual, has_solve = j + 1 < B.slots || B.last_solve;
    if (has_residual) {
      if (S.entered >= max_iterations) return false;
      if (seen_res >= n_res) return false;                 // the gate was open, so the part ran
      ++seen_res; ++S.entered; S.l2.push_back(std::sqrt(rec[kNewtonHead + 3 * j])); S.solve_pending = true;
      if (seen_res == n_res && code == kNewtonConverged) { closed = true; S.solve_pending = false; S.code = kNewtonConverged; break; }
    }
    if (has_solve) {
      if (!S.solve_pending) return false;
      S.res.push_back(std::sqrt(rec[kNewtonHead + 3 * j + 1])); S.bn.push_back(std::sqrt(rec[kNewtonHead + 3 * j + 2]));
      if (seen_ok < n_ok) { ++seen_ok; ++S.solves; S.solve_pending = false; }
      else if (code == kNewtonFallback) { closed = true; S.code = kNewtonFallback; }
      else return false;
    }
  }
  if (seen_res != n_res || seen_ok != n_ok) return false;
  if (!closed && code != kNewtonOpen) return false;
  if (closed) S.finished = true;
  else if (S.entered >= max_iterations && !S.solve_pending) S.finished = true;      // the cap: the loop ends behind the solve of its last iteration
  if (S.finished && S.code != kNewtonFallback) S.pinf = rec[3];
  return true;
}

}  // namespace poro
