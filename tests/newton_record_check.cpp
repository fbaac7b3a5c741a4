// Stand-alone check of csrc/newton_record.hpp (host-only): the batches the pressure Newton loop plans and what the host rebuilds from their records, against the
// per-call loop of PoroelasticityFSS.h:358-380 on made-up residual histories: convergence at every iteration, every cap, every prediction, a failed check at every solve.
// A small model of the device fills the record the way the gated kernels do.  Prints "newton_record_check ok".  Built by tests/test_newton_record_cpu.py with
// -fsanitize=address,undefined
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "newton_record.hpp"

using namespace poro;

struct Scenario { std::vector<double> l2; double tol; int fail_at; /* the solve of this iteration (1-based) fails its check; 0: none */ int max_it; };
struct Expected { int entered = 0, solves = 0, code = kNewtonOpen; std::vector<double> l2; };

static double l2_of(const Scenario &sc, int it) { return it <= (int)sc.l2.size() ? sc.l2[it - 1] : sc.l2.back(); }

// the loop as the host runs it call by call
static Expected per_call(const Scenario &sc) {
  Expected E;
  while (E.entered < sc.max_it) {
    ++E.entered; E.l2.push_back(l2_of(sc, E.entered));
    if (E.l2.back() < sc.tol) { E.code = kNewtonConverged; return E; }
    if (E.entered == sc.fail_at) { E.code = kNewtonFallback; return E; }
    ++E.solves;
  }
  return E;
}

// the device: the gated kernels of one batch, starting behind iteration `entered`
static void device_batch(const Scenario &sc, const NewtonBatch &B, int entered, double *rec) {
  for (int k = 0; k < kNewtonRecord; ++k) rec[k] = 0;
  bool closed = false;
  for (int j = 0; j < B.slots; ++j) {
    if ((j > 0 || B.first_residual) && !closed) {
      ++entered; const double l2 = l2_of(sc, entered);
      rec[kNewtonHead + 3 * j] = l2 * l2; rec[0] += 1;
      if (std::sqrt(l2 * l2) < sc.tol) { rec[2] = kNewtonConverged; closed = true; }
    }
    if ((j + 1 < B.slots || B.last_solve) && !closed) {
      rec[kNewtonHead + 3 * j + 1] = 1e-20 * entered; rec[kNewtonHead + 3 * j + 2] = 4.0 * entered;
      if (entered == sc.fail_at) { rec[2] = kNewtonFallback; closed = true; } else rec[1] += 1;
    }
  }
  rec[3] = 7.5;
}

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s (line %d): conv %d fail %d cap %d pred %d\n", #x, __LINE__, conv, fail_at, cap, pred); ++failures; } } while (0)

int main() {
  int cases = 0, most_batches = 0;
  for (int conv = 1; conv <= 9; ++conv)            // the first iteration whose residual is below the tolerance
    for (int fail_at = 0; fail_at <= 6; ++fail_at)
      for (int cap = 1; cap <= 10; ++cap)
        for (int pred = 0; pred <= 9; ++pred) {
          Scenario sc; sc.tol = 1e-8; sc.fail_at = fail_at; sc.max_it = cap;
          for (int it = 1; it <= conv; ++it) sc.l2.push_back(it < conv ? 1.0 / it : 0.25e-8);      // (0.25e-8 = sqrt of its own square exactly enough: 2^-2 scaling)
          const Expected E = per_call(sc);
          NewtonState S; int batches = 0;
          while (!S.finished) {
            const NewtonBatch B = newton_plan_batch(S, cap, pred);
            CHECK(B.slots >= 1 && B.slots <= kNewtonSlots);
            if (B.slots < 1) break;
            double rec[kNewtonRecord];
            device_batch(sc, B, S.entered, rec);
            const bool ok = newton_absorb(S, B, rec, cap);
            CHECK(ok);
            if (!ok || ++batches > 20) break;
          }
          CHECK(S.finished);
          CHECK(S.entered == E.entered && S.solves == E.solves && S.code == E.code);
          CHECK(S.l2.size() == E.l2.size());
          for (size_t i = 0; i < S.l2.size() && i < E.l2.size(); ++i) CHECK(S.l2[i] == std::sqrt(E.l2[i] * E.l2[i]));
          CHECK((int)S.res.size() == E.solves + (E.code == kNewtonFallback ? 1 : 0) && S.res.size() == S.bn.size());
          for (size_t k = 0; k < S.bn.size(); ++k) CHECK(S.bn[k] == std::sqrt(4.0 * (k + 1)));      // the k-th check belongs to iteration k + 1
          if (E.code != kNewtonFallback) CHECK(S.pinf == 7.5);
          if (pred == E.entered && E.entered <= kNewtonSlots && E.code != kNewtonFallback) CHECK(batches == 1);      // a right prediction: one wait
          if (batches > most_batches) most_batches = batches;
          ++cases;
        }
  // records that contradict their batch are refused, not read past
  {
    const int conv = 0, fail_at = 0, cap = 5, pred = 0;
    NewtonState S; NewtonBatch B = newton_plan_batch(S, cap, pred);
    double rec[kNewtonRecord] = {0};
    rec[0] = 5; CHECK(!newton_absorb(S, B, rec, cap));                                      // more residuals than slots
    S = NewtonState(); rec[0] = 1; rec[1] = 1; rec[2] = 1; CHECK(!newton_absorb(S, B, rec, cap));      // converged at the first residual, yet a solve counted
    S = NewtonState(); rec[0] = 1; rec[1] = 0; rec[2] = 7; CHECK(!newton_absorb(S, B, rec, cap));      // no such code
    S = NewtonState(); rec[0] = 0.5; rec[2] = 0; CHECK(!newton_absorb(S, B, rec, cap));               // not a count
    S = NewtonState(); rec[0] = 1; rec[1] = 0; rec[2] = 0; CHECK(!newton_absorb(S, B, rec, cap));      // gate open, but the first solve neither counted nor failed
    NewtonBatch bad; bad.slots = kNewtonSlots + 1; S = NewtonState(); CHECK(!newton_absorb(S, bad, rec, cap));
  }
  std::printf("%d cases, at most %d batches per loop\n", cases, most_batches);
  if (failures) { std::printf("%d failures\n", failures); return 1; }
  std::printf("newton_record_check ok\n");
  return 0;
}
