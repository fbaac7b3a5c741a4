// Stand-alone check of host/run_controls.hpp: poro_host_run_options -> RunControls, member by member.  Every member of the options struct, set to a value of its own,
// changes the RunControls member of the same name and no other; the defaulted struct gives RunControls{}; refine_every < 0 is refused; a Chebyshev ratio of 12.5 and a
// degree of 300 arrive as given.  Prints the layout of the C struct ("sizeof N", "offsetof NAME N") for tests/test_run_options_cpu.py, which holds it against the ctypes
// mirror, then "run_options_check ok".  Built by that test with -fsanitize=address,undefined and run directly; the exit code names the check that failed.
#include <cstddef>
#include <cstdio>
#include <functional>
#include <string>
#include <utility>
#include <vector>
#include "../poroelasticity_dealii_amd/host/run_controls.hpp"

using poro_host::RunControls;

// every member of the options struct, once
#define OPTION_MEMBERS(X) \
  X(p_init) X(time_step) X(n_steps) X(fss_tol) X(pressure_tol) X(max_fss_iterations) X(max_pressure_iterations) X(abs_tol_u) X(rel_tol_u) X(max_iter) X(preconditioner) \
  X(stop_rule_u) X(preconditioner_p) X(coupled_fss) X(incremental_strain) X(atomic_scatter) X(fdm_fp32) X(hybrid_operator) X(fdm_per_direction) X(moduli_structured) \
  X(chebyshev_degree) X(chebyshev_ratio) X(refine_every) X(refine_fraction) X(coarsen_fraction)

static std::string text(double v) { char b[64]; std::snprintf(b, sizeof b, "%a", v); return b; }      // exact
static std::string text(int v) { return std::to_string(v); }
static std::string text(bool v) { return v ? "1" : "0"; }
static std::string text(const std::string &v) { return "'" + v + "'"; }

// every member of RunControls by name, rendered exactly.  The binding names them all: a member added to RunControls stops this file from compiling until it is listed
static std::vector<std::pair<std::string, std::string>> members(const RunControls &r) {
  const auto &[p_init, time_step, n_steps, fss_tol, pressure_tol, max_fss_iterations, max_pressure_iterations, abs_tol_u, rel_tol_u, max_iter, stop_rule_u, preconditioner,
               coupled_fss, incremental_strain, corrected_postprocessing, output_dir, chebyshev_degree, chebyshev_ratio, preconditioner_p, fdm_fp32, fdm_per_direction,
               moduli_structured, atomic_scatter, hybrid_operator, refine_every, refine_fraction, coarsen_fraction] = r;
#define M(name) {#name, text(name)}
  return {M(p_init), M(time_step), M(n_steps), M(fss_tol), M(pressure_tol), M(max_fss_iterations), M(max_pressure_iterations), M(abs_tol_u), M(rel_tol_u), M(max_iter),
          M(stop_rule_u), M(preconditioner), M(coupled_fss), M(incremental_strain), M(corrected_postprocessing), M(output_dir), M(chebyshev_degree), M(chebyshev_ratio),
          M(preconditioner_p), M(fdm_fp32), M(fdm_per_direction), M(moduli_structured), M(atomic_scatter), M(hybrid_operator), M(refine_every), M(refine_fraction),
          M(coarsen_fraction)};
#undef M
}

struct Case { const char *name; std::function<void(poro_host_run_options &)> set; std::string want; };

int main() {
  const auto defaults = members(RunControls{});
  {  // zero-initialised, then defaulted: exactly RunControls{}
    poro_host_run_options o{};
    o = poro_host::default_run_options();
    if (members(poro_host::to_run_controls(o)) != defaults) return 1;
  }
  {  // the binding names every member of the options struct: one added there stops this file from compiling until OPTION_MEMBERS and the cases list it
    const auto [p_init, time_step, n_steps, fss_tol, pressure_tol, max_fss_iterations, max_pressure_iterations, abs_tol_u, rel_tol_u, max_iter, preconditioner, stop_rule_u,
                preconditioner_p, coupled_fss, incremental_strain, atomic_scatter, fdm_fp32, hybrid_operator, fdm_per_direction, moduli_structured, chebyshev_degree,
                chebyshev_ratio, refine_every, refine_fraction, coarsen_fraction] = poro_host::default_run_options();
    (void)p_init; (void)time_step; (void)n_steps; (void)fss_tol; (void)pressure_tol; (void)max_fss_iterations; (void)max_pressure_iterations; (void)abs_tol_u; (void)rel_tol_u;
    (void)max_iter; (void)preconditioner; (void)stop_rule_u; (void)preconditioner_p; (void)coupled_fss; (void)incremental_strain; (void)atomic_scatter; (void)fdm_fp32;
    (void)hybrid_operator; (void)fdm_per_direction; (void)moduli_structured; (void)chebyshev_degree; (void)chebyshev_ratio; (void)refine_every; (void)refine_fraction;
    (void)coarsen_fraction;
  }
  // one value per member, different from the default and from every other case's
#define CASE(name, value) {#name, [](poro_host_run_options &o) { o.name = value; }, text(decltype(RunControls::name)(value))}
  const std::vector<Case> cases = {
      CASE(p_init, 1.5e6), CASE(time_step, 7.25), CASE(n_steps, 3), CASE(fss_tol, 1e-5), CASE(pressure_tol, 2e-6), CASE(max_fss_iterations, 11), CASE(max_pressure_iterations, 13),
      CASE(abs_tol_u, 3e-10), CASE(rel_tol_u, 4e-7), CASE(max_iter, 1717), CASE(preconditioner, PORO_PREC_FDM), CASE(stop_rule_u, PORO_STOP_REDUCTION),
      CASE(preconditioner_p, PORO_PREC_TWO_LEVEL), CASE(coupled_fss, 1), CASE(incremental_strain, 1), CASE(atomic_scatter, 1), CASE(fdm_fp32, 1), CASE(hybrid_operator, 1),
      CASE(fdm_per_direction, 1), CASE(moduli_structured, 1), CASE(chebyshev_degree, 300), CASE(chebyshev_ratio, 12.5), CASE(refine_every, 5), CASE(refine_fraction, 0.35),
      CASE(coarsen_fraction, 0.15)};
#undef CASE
  size_t n_members = 0;
#define COUNT(name) ++n_members;
  OPTION_MEMBERS(COUNT)
#undef COUNT
  if (cases.size() != n_members) return 2;
  for (size_t k = 0; k < cases.size(); ++k) {
    poro_host_run_options o = poro_host::default_run_options();
    cases[k].set(o);
    const auto got = members(poro_host::to_run_controls(o));
    int changed = 0;
    for (size_t m = 0; m < got.size(); ++m) {
      if (got[m].first == cases[k].name) { if (got[m].second != cases[k].want || got[m].second == defaults[m].second) return 10 + (int)k; ++changed; }
      else if (got[m].second != defaults[m].second) return 50 + (int)k;      // another member moved
    }
    if (changed != 1) return 90;
  }
  {  // as given: no clipping to 8 / 15 bits, no rounding
    poro_host_run_options o = poro_host::default_run_options();
    o.chebyshev_ratio = 12.5; o.chebyshev_degree = 300;
    const RunControls rc = poro_host::to_run_controls(o);
    if (rc.chebyshev_ratio != 12.5 || rc.chebyshev_degree != 300) return 3;
  }
  {  // the refusal
    poro_host_run_options o = poro_host::default_run_options();
    o.refine_every = -1;
    bool refused = false;
    try { poro_host::to_run_controls(o); } catch (const std::runtime_error &) { refused = true; }
    if (!refused) return 4;
  }
  std::printf("sizeof %zu\n", sizeof(poro_host_run_options));
#define OFFSET(name) std::printf("offsetof %s %zu\n", #name, offsetof(poro_host_run_options, name));
  OPTION_MEMBERS(OFFSET)
#undef OFFSET
  std::printf("run_options_check ok\n");
  return 0;
}
