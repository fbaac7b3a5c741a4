// Driver executable: `poro_run input.data [--mesh domain.msh] [--degree 1|2] [--matrix-free] [--ssor | --chebyshev | --block-fdm] [--steps N] [--output DIR [--darcy-output] [--stress-output]] [--corrected-output] [--flow-balance] [--force-balance] [--mohr-coulomb COHESION,FRICTION_DEG] [--coupled-fss] [--incremental-strain] [--pressure-bc LABEL=VALUE ...] [--permeability-layers TOP=VALUE[,TOP=VALUE...]] [--permeability-tensor-layers TOP=KX:KY[:KZ][,...]] [--moduli-layers TOP=YOUNG:POISSON[,...]] [--atomic-scatter] [--hybrid-operator] [--fdm-fp32] [--fdm-per-direction] [--moduli-structured] [--refine-every N [--refine-fraction f] [--coarsen-fraction f]]`.
// Stands in for the reference's missing code/source/Runner.cpp (code/CMakeLists.txt:8): argv[1] is the
// parameter file (parse_command_line.h:5-27); the mesh is create_mesh()'s colorized box refined
// `Initial refinement level` times (PoroelasticityFSS.h:418-435) unless --mesh names a Gmsh file
// (read_mesh, :438-445).  --output DIR writes DIR/solution-NNNN.vtk after every step like output_results (:227-291).
// --pressure-bc LABEL=VALUE (repeatable; an extension, the reference has no pressure boundary conditions) prescribes the pressure on a boundary label, e.g. a drained face
// `--pressure-bc 3=0`; the run then also prints which preconditioners the pressure and projection systems got.
// --permeability-layers TOP=VALUE[,TOP=VALUE...] (an extension: the reference's permeability is one constant) sets k / mu layer by layer along the slowest direction, in the
// units of k / mu: a cell takes the VALUE of the first layer whose TOP is >= the coordinate of its centre (e.g. a caprock over a reservoir: `0=1e-11,5=1e-14` on the box
// [-5, 5]^3).  --fastest then takes the fast diagonalisation for the pressure system on boxes and Jacobi elsewhere; the run prints the choice.
// --permeability-tensor-layers TOP=KX:KY[:KZ][,TOP=KX:KY[:KZ]...] (an extension likewise) sets the diagonal tensor diag(kx, ky[, kz]) / mu layer by layer in the same way: one
// value per direction of the problem (KZ in 3D only), e.g. a sediment with kv = kh / 100: `5=1e-11:1e-11:1e-13`.  Not together with --permeability-layers.
// --moduli-layers TOP=YOUNG:POISSON[,TOP=YOUNG:POISSON...] (an extension likewise) sets Young's modulus and Poisson's ratio layer by layer along the slowest direction, the
// layers chosen by cell centres in the same way; lambda and G follow by the parameter file's formulas.  On a box the displacement operator then runs the general cell loop;
// --fastest takes the fast diagonalisation (line-solve form) on boxes and Chebyshev elsewhere; the run prints the field's kind and the choice, also after every adapt.
// --flow-balance (an extension: the reference computes no flow) prints after the log of every step one line with the six terms of the discrete fluid balance
// (include/poroel_hip.h, poro_pres_flow_balance), the conservative outflow and the face-integrated discharge per prescribed label and the imbalance against its bound
// sqrt(n) * residual_l2, and at the end the cumulative volumes.  --darcy-output (with --output) appends the Darcy velocity per cell to every VTK file.  Without the two
// options the log and the files are what they were.
// --stress-output (with --output; an extension likewise) appends to every VTK file, behind what --darcy-output appends, the effective and the total stress per cell and the
// Mohr-Coulomb function and von Mises stress (include/poroel_hip.h, poro_disp_cell_stress / poro_disp_cell_measures).  --mohr-coulomb COHESION,FRICTION_DEG sets the
// criterion (without it f = 0) and prints after every step's log max f, its cell and the number of failing cells.  --force-balance prints after every step's log one line
// with the reaction per displacement condition, per component the reaction, the applied loads and the closure against its bound sqrt(n) * residual_l2.
// --refine-every N adapts the mesh every N-th step like refine_mesh (:333-340, :447-498; the reference hard-wires N = 5) on the box with ONE level of refinement
// (the analogue of `Max refinement level = 1`): the box is then built as a refined box with an empty mask, i.e. as a general mesh with the two-level coarse space.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <iostream>
#include <string>
#include "input_data.hpp"
#include "mesh.hpp"
#include "problem.hpp"

using namespace poro_host;

static const char *const kUsage = "usage: poro_run input.data [--mesh domain.msh] [--degree 1|2] [--device N] [--matrix-free] [--ssor | --chebyshev | --block-fdm | --two-level | --fastest] [--steps N] [--output DIR [--darcy-output] [--stress-output]] "
                                  "[--corrected-output] [--flow-balance] [--force-balance] [--mohr-coulomb COHESION,FRICTION_DEG] [--coupled-fss] [--incremental-strain] [--pressure-bc LABEL=VALUE ...] [--permeability-layers TOP=VALUE[,TOP=VALUE...]] [--permeability-tensor-layers TOP=KX:KY[:KZ][,...]] [--moduli-layers TOP=YOUNG:POISSON[,...]] [--atomic-scatter] [--hybrid-operator] [--fdm-fp32] [--fdm-per-direction] [--moduli-structured] "
                                  "[--gravity GX,GY[,GZ]] [--fluid-density RHO] [--density-layers TOP=RHO[,TOP=RHO...]] [--hydrostatic-init] "
                                  "[--refine-every N [--refine-fraction f] [--coarsen-fraction f]]";

// TOP=V[:V...][,TOP=V[:V...]...], one array of `fields` per number of an item (the tops first): appends every item.  False unless every item has that shape, every number
// is read whole and the tops ascend (from the last one the array holds already)
static bool parse_layers(const std::string &arg, std::initializer_list<std::vector<double> *> fields) {
  for (size_t at = 0, comma; at <= arg.size(); at = comma + 1) {
    comma = std::min(arg.find(',', at), arg.size());
    std::string rest = arg.substr(at, comma - at); size_t k = 0;
    for (std::vector<double> *out : fields) {
      const size_t end = ++k == fields.size() ? rest.size() : rest.find(k == 1 ? '=' : ':');      // (the last number takes what is left)
      const std::string text = rest.substr(0, end); char *stop = nullptr; const double v = std::strtod(text.c_str(), &stop);
      if (end == std::string::npos || text.empty() || *stop || (k == 1 && !out->empty() && !(v > out->back()))) return false;
      out->push_back(v); rest.erase(0, end + 1);
    }
  }
  return true;
}
static bool positive(double v) { return v > 0 && std::isfinite(v); }

int main(int argc, char **argv) {
  if (argc < 2) { std::cerr << "specify the file name" << std::endl << kUsage << std::endl; return 1; }   // parse_command_line.h:9-13 (the usage line is this driver's)
  std::string mesh_file; int degree = 2, op = PORO_OP_CSR, steps = -1, device = 0;
  RunControls rc;      // the options go straight into it; the parameter file adds its own below
  std::vector<int32_t> pressure_labels; std::vector<double> pressure_values;
  std::vector<double> layer_top, layer_value;
  std::vector<double> tensor_top, tensor_k[3];
  std::vector<double> moduli_top, moduli_young, moduli_poisson;
  std::vector<double> gravity, density_top, density_value; double fluid_density = 0; bool hydrostatic_init = false;
  bool flow_balance = false, darcy_output = false;
  bool force_balance = false, stress_output = false, mohr_coulomb = false; double mc_cohesion = 0, mc_friction_deg = 0;
  for (int i = 2; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--mesh") && i + 1 < argc) mesh_file = argv[++i];
    else if (!std::strcmp(argv[i], "--degree") && i + 1 < argc) degree = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--steps") && i + 1 < argc) steps = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--device") && i + 1 < argc) device = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--matrix-free")) op = PORO_OP_MATRIX_FREE;
    else if (!std::strcmp(argv[i], "--output") && i + 1 < argc) rc.output_dir = argv[++i];
    else if (!std::strcmp(argv[i], "--corrected-output")) rc.corrected_postprocessing = true;
    else if (!std::strcmp(argv[i], "--darcy-output")) darcy_output = true;       // with --output: one Darcy velocity per cell appended to every file (CELL_DATA / VECTORS darcy_velocity)
    else if (!std::strcmp(argv[i], "--stress-output")) stress_output = true;     // with --output: effective / total stress, Mohr-Coulomb function and von Mises stress per cell appended to every file
    else if (!std::strcmp(argv[i], "--force-balance")) force_balance = true;     // one line per step with the support reactions, the loads and the closure
    else if (!std::strcmp(argv[i], "--mohr-coulomb") && i + 1 < argc) {          // COHESION,FRICTION_DEG: the criterion of the failure measure; one line per step with max f, its cell, the failing cells
      const char *arg = argv[++i], *comma = std::strchr(arg, ','); char *end = nullptr, *end2 = nullptr;
      mc_cohesion = std::strtod(arg, &end); mc_friction_deg = comma ? std::strtod(comma + 1, &end2) : 0.0;
      if (!comma || end != comma || comma == arg || !end2 || end2 == comma + 1 || *end2 || !(mc_cohesion >= 0) || !(mc_friction_deg >= 0 && mc_friction_deg < 90)) {
        std::cerr << "--mohr-coulomb needs COHESION,FRICTION_DEG with COHESION >= 0 and 0 <= FRICTION_DEG < 90, got " << arg << std::endl; return 1;
      }
      mohr_coulomb = true;
    }
    else if (!std::strcmp(argv[i], "--flow-balance")) flow_balance = true;       // one line per step with the terms of the discrete fluid balance, the cumulative volumes at the end
    else if (!std::strcmp(argv[i], "--incremental-strain")) rc.incremental_strain = true;   // storage term against the previous step instead of the initial state
    else if (!std::strcmp(argv[i], "--coupled-fss")) rc.coupled_fss = true;    // restore get_volumetric_strain() inside the fixed-stress loop (:399)
    else if (!std::strcmp(argv[i], "--ssor")) rc.preconditioner = PORO_PREC_SSOR;   // the reference's PreconditionSSOR instead of Jacobi
    else if (!std::strcmp(argv[i], "--chebyshev")) rc.preconditioner = PORO_PREC_CHEBYSHEV;   // polynomial preconditioner (any mesh / operator)
    else if (!std::strcmp(argv[i], "--block-fdm")) rc.preconditioner = PORO_PREC_FDM;         // block fast diagonalisation (uniform boxes with face-wise Dirichlet data)
    else if (!std::strcmp(argv[i], "--two-level")) rc.preconditioner = PORO_PREC_TWO_LEVEL;   // Jacobi + block fast diagonalisation of the underlying / auxiliary box (refined boxes, rectangle-filling Gmsh meshes)
    else if (!std::strcmp(argv[i], "--atomic-scatter")) rc.atomic_scatter = true;   // general meshes, --matrix-free: one launch per operator application with fp64 atomic adds (last bits differ from run to run)
    else if (!std::strcmp(argv[i], "--hybrid-operator")) rc.hybrid_operator = true; // refined boxes (--refine-every), --matrix-free: the box's structured kernel + the general kernels on the fine cells only; no effect on box-tagged meshes, an error where the mesh cannot take it
    else if (!std::strcmp(argv[i], "--fdm-fp32")) rc.fdm_fp32 = true;               // with --block-fdm / --fastest: fp32 transforms in the displacement system's block FDM (single-rank 3D octant form; elsewhere no effect)
    else if (!std::strcmp(argv[i], "--fdm-per-direction")) rc.fdm_per_direction = true;   // with --block-fdm / --fastest: the per-direction form of the block FDM (single-rank 3D boxes whose directions are not all mirror-symmetric; elsewhere no effect)
    else if (!std::strcmp(argv[i], "--moduli-structured")) rc.moduli_structured = true;   // with --moduli-layers and --matrix-free: the structured operator on uniform 3D boxes whose layers follow the cell layers of z (elsewhere no effect)
    else if (!std::strcmp(argv[i], "--refine-every") && i + 1 < argc) rc.refine_every = std::atoi(argv[++i]);            // 0 = never (default)
    else if (!std::strcmp(argv[i], "--refine-fraction") && i + 1 < argc) rc.refine_fraction = std::atof(argv[++i]);
    else if (!std::strcmp(argv[i], "--coarsen-fraction") && i + 1 < argc) rc.coarsen_fraction = std::atof(argv[++i]);
    else if (!std::strcmp(argv[i], "--pressure-bc") && i + 1 < argc) {           // prescribed pressure VALUE on the boundary LABEL (one rank; boxes: whole faces, which keeps the fast diagonalisation)
      const char *arg = argv[++i], *eq = std::strchr(arg, '='); char *end = nullptr, *end2 = nullptr;
      const long label = std::strtol(arg, &end, 10); const double value = eq ? std::strtod(eq + 1, &end2) : 0.0;
      if (!eq || end != eq || eq == arg || !end2 || end2 == eq + 1 || *end2 || label < 0) { std::cerr << "--pressure-bc needs LABEL=VALUE, got " << arg << std::endl; return 1; }
      pressure_labels.push_back((int32_t)label); pressure_values.push_back(value);
    }
    else if (!std::strcmp(argv[i], "--permeability-layers") && i + 1 < argc) {   // k / mu by layers of the slowest direction, bottom to top
      const char *arg = argv[++i];
      if (!parse_layers(arg, {&layer_top, &layer_value}) || !std::all_of(layer_value.begin(), layer_value.end(), positive)) {
        std::cerr << "--permeability-layers needs TOP=VALUE[,TOP=VALUE...] with ascending tops and positive values, got " << arg << std::endl; return 1;
      }
    }
    else if (!std::strcmp(argv[i], "--permeability-tensor-layers") && i + 1 < argc) {   // diag(kx, ky[, kz]) / mu by layers of the slowest direction, bottom to top
      const char *arg = argv[++i];
      std::vector<double> top3, k3[3], top2, k2[2];             // every item with three values, or every item with two
      const bool three = parse_layers(arg, {&top3, &k3[0], &k3[1], &k3[2]}), two = !three && parse_layers(arg, {&top2, &k2[0], &k2[1]});
      bool ok = (three || two) && tensor_top.empty();
      if (three) { tensor_top = top3; for (int d = 0; d < 3; ++d) tensor_k[d] = k3[d]; }
      if (two) { tensor_top = top2; for (int d = 0; d < 2; ++d) tensor_k[d] = k2[d]; }
      for (int d = 0; d < 3; ++d) ok = ok && std::all_of(tensor_k[d].begin(), tensor_k[d].end(), positive);
      if (!ok) { std::cerr << "--permeability-tensor-layers needs (once) TOP=KX:KY[:KZ][,TOP=KX:KY[:KZ]...] with ascending tops and positive values, got " << arg << std::endl; return 1; }
    }
    else if (!std::strcmp(argv[i], "--moduli-layers") && i + 1 < argc) {   // Young's modulus and Poisson's ratio by layers of the slowest direction, bottom to top
      const char *arg = argv[++i];
      if (!parse_layers(arg, {&moduli_top, &moduli_young, &moduli_poisson}) || !std::all_of(moduli_young.begin(), moduli_young.end(), positive) ||
          !std::all_of(moduli_poisson.begin(), moduli_poisson.end(), [](double v) { return v > -1.0 && v < 0.5; })) {
        std::cerr << "--moduli-layers needs TOP=YOUNG:POISSON[,TOP=YOUNG:POISSON...] with ascending tops, YOUNG > 0 and POISSON in (-1, 0.5), got " << arg << std::endl; return 1;
      }
    }
    else if (!std::strcmp(argv[i], "--gravity") && i + 1 < argc) {         // the gravity vector, one component per dimension: body force rho_b g (Properties/Bulk density, or --density-layers)
      const char *arg = argv[++i]; gravity.clear();
      for (const char *at = arg;;) { char *end = nullptr; const double v = std::strtod(at, &end); if (end == at || !std::isfinite(v)) { gravity.clear(); break; } gravity.push_back(v); if (!*end) break; if (*end != ',') { gravity.clear(); break; } at = end + 1; }
      if (gravity.size() != 2 && gravity.size() != 3) { std::cerr << "--gravity needs GX,GY[,GZ], got " << arg << std::endl; return 1; }
    }
    else if (!std::strcmp(argv[i], "--fluid-density") && i + 1 < argc) {   // with --gravity: the Darcy gravity flux, q = -k / mu (grad p - RHO g)
      const char *arg = argv[++i]; char *end = nullptr; fluid_density = std::strtod(arg, &end);
      if (end == arg || *end || !(std::isfinite(fluid_density) && fluid_density >= 0)) { std::cerr << "--fluid-density needs a density >= 0, got " << arg << std::endl; return 1; }
    }
    else if (!std::strcmp(argv[i], "--density-layers") && i + 1 < argc) {  // bulk density by layers of the slowest direction, bottom to top
      const char *arg = argv[++i];
      if (!parse_layers(arg, {&density_top, &density_value}) || !std::all_of(density_value.begin(), density_value.end(), positive)) {
        std::cerr << "--density-layers needs TOP=RHO[,TOP=RHO...] with ascending tops and positive values, got " << arg << std::endl; return 1;
      }
    }
    else if (!std::strcmp(argv[i], "--hydrostatic-init")) hydrostatic_init = true;   // with --gravity and --fluid-density: start from the initial pressure at the top and the hydrostatic pressure below
    else if (!std::strcmp(argv[i], "--fastest")) rc.preconditioner = -1;                      // the strongest preconditioner the mesh supports: block FDM, else two-level, else Chebyshev
    else { std::cerr << "unknown option " << argv[i] << std::endl; return 1; }
  }
  if (rc.fdm_fp32 && rc.preconditioner != PORO_PREC_FDM && rc.preconditioner != -1) { std::cerr << "--fdm-fp32 needs --block-fdm or --fastest" << std::endl; return 1; }
  if (rc.fdm_per_direction && rc.preconditioner != PORO_PREC_FDM && rc.preconditioner != -1) { std::cerr << "--fdm-per-direction needs --block-fdm or --fastest" << std::endl; return 1; }
  if (!layer_top.empty() && !tensor_top.empty()) { std::cerr << "--permeability-tensor-layers and --permeability-layers exclude each other (a context holds the scalar field or the tensor)" << std::endl; return 1; }
  if (rc.refine_every < 0) { std::cerr << "--refine-every needs a non-negative step count" << std::endl; return 1; }
  if (rc.refine_every > 0 && !mesh_file.empty()) { std::cerr << "--refine-every adapts boxes only (not --mesh)" << std::endl; return 1; }
  try {
    input_data::InputDataPoroel data;
    data.read_input_file(argv[1]);
    ProblemData P;
    P.bc.dirichlet_labels.assign(data.displacement_boundary_labels.begin(), data.displacement_boundary_labels.end());
    P.bc.dirichlet_components.assign(data.displacement_boundary_components.begin(), data.displacement_boundary_components.end());
    P.bc.dirichlet_values = data.displacement_boundary_values;
    P.bc.neumann_labels.assign(data.stress_boundary_labels.begin(), data.stress_boundary_labels.end());
    P.bc.neumann_components.assign(data.stress_boundary_components.begin(), data.stress_boundary_components.end());
    P.bc.neumann_values = data.stress_boundary_values;
    P.bc.pressure_labels = pressure_labels; P.bc.pressure_values = pressure_values;
    P.mat = data.material();
    if (!mesh_file.empty()) { P.mesh = read_gmsh22(mesh_file); P.finalize(degree); attach_auxiliary_box(P, degree); }   // (coarse space of --two-level / --fastest where the mesh fills a rectangle)
    else {
      int n[3] = {1, 1, 1}; double size[3] = {1, 1, 1};
      for (int d = 0; d < data.dim; ++d) { n[d] = 1 << data.initial_refinement_level; size[d] = data.domain_size.at(d); }
      if (rc.refine_every > 0) build_refined_box_problem_mask(P, data.dim, n, size, degree, std::vector<uint8_t>((size_t)n[0] * n[1] * n[2], 0));
      else build_box_problem(P, data.dim, n, size, degree);
    }
    if (!layer_top.empty()) P.set_permeability_layers((int)layer_top.size(), layer_top.data(), layer_value.data());
    if (!tensor_top.empty()) {
      if ((data.dim == 3) != !tensor_k[2].empty()) throw std::runtime_error("--permeability-tensor-layers: a " + std::to_string(data.dim) + "D problem needs " + (data.dim == 3 ? "TOP=KX:KY:KZ" : "TOP=KX:KY") + " layers");
      P.set_permeability_tensor_layers((int)tensor_top.size(), tensor_top.data(), tensor_k[0].data(), tensor_k[1].data(), data.dim == 3 ? tensor_k[2].data() : nullptr);
    }
    if (!moduli_top.empty()) P.set_moduli_layers((int)moduli_top.size(), moduli_top.data(), moduli_young.data(), moduli_poisson.data());
    if (!gravity.empty()) {
      if ((int)gravity.size() != data.dim) throw std::runtime_error("--gravity: a " + std::to_string(data.dim) + "D problem needs " + std::to_string(data.dim) + " components");
      P.set_gravity(gravity.data(), fluid_density, data.bulk_density); P.hydrostatic_init = hydrostatic_init;
    }
    if (!density_top.empty()) P.set_density_layers((int)density_top.size(), density_top.data(), density_value.data());
    rc.p_init = data.p_init; rc.time_step = data.time_step; rc.fss_tol = data.fss_tol; rc.pressure_tol = data.pressure_tol;
    rc.max_fss_iterations = data.max_fss_iterations; rc.max_pressure_iterations = data.max_pressure_iterations;
    int n_steps = 0; for (double t = 0; t < data.t_max; t += data.time_step) ++n_steps;   // while (time < t_max) (:327)
    rc.n_steps = steps >= 0 ? steps : n_steps;
    std::vector<double> trace(8 * (size_t)(1 + rc.n_steps * rc.max_fss_iterations));
    int rows;
    std::vector<std::string> flow_lines;      // --flow-balance: one line per step, then the totals
    std::vector<std::string> force_lines, failure_lines;   // --force-balance, --mohr-coulomb: one line per step
    std::cout << "starting time loop" << std::endl << "time max " << data.t_max << std::endl;   // :325-326
    static const char *const prec_name[] = {"none", "Jacobi", "SSOR", "FDM", "ILU0", "Chebyshev", "two-level"};
    auto go = [&](auto &prob) {
      auto moduli_line = [&](std::ostream &os) {            // the field's kind on the present context and the displacement preconditioner chosen for it
        int32_t kind = 0;
        if (poro_ctx_get_cell_moduli(prob.context(), nullptr, nullptr, 0, &kind) != 0) throw std::runtime_error(poro_last_error());
        os << "moduli layers: " << moduli_top.size() << ", field kind " << kind << "; displacement preconditioner: " << prec_name[prob.displacement_solver.control.preconditioner];
        if (rc.moduli_structured) {           // (only with the option) what an operator application runs on the present context
          int32_t req = 0, eff = 0;
          if (poro_ctx_get_moduli_operator(prob.context(), &req, &eff) != 0) throw std::runtime_error(poro_last_error());
          os << "; moduli operator: " << (eff == PORO_MODULI_OP_STRUCTURED ? "structured" : "cell loop");
        }
      };
      auto tensor_line = [&](std::ostream &os) {            // likewise the tensor's kind and the pressure preconditioner chosen for it
        int32_t kind = 0;
        if (poro_ctx_get_cell_permeability_tensor(prob.context(), nullptr, 0, &kind) != 0) throw std::runtime_error(poro_last_error());
        os << "permeability tensor layers: " << tensor_top.size() << ", field kind " << kind << "; pressure preconditioner: " << prec_name[prob.pressure_solver.control.preconditioner];
      };
      auto gravity_line = [&](std::ostream &os) {           // what the present context holds
        double g[3] = {0, 0, 0}, rho_b = 0, rho_f = 0; int32_t on = 0, kind = 0;
        if (poro_ctx_get_gravity(prob.context(), g, &rho_b, &rho_f, &on) != 0 || poro_ctx_get_cell_density(prob.context(), nullptr, 0, &kind) != 0) throw std::runtime_error(poro_last_error());
        os << "gravity: " << (on ? "on" : "off") << ", g = (" << g[0] << ", " << g[1]; if (data.dim == 3) os << ", " << g[2];
        os << "), bulk density " << rho_b << ", density layers: " << density_top.size() << " (field kind " << kind << "), fluid density " << rho_f << ", hydrostatic start: " << (hydrostatic_init ? "yes" : "no");
      };
      if (!pressure_labels.empty() || !layer_top.empty() || !moduli_top.empty() || !tensor_top.empty() || !gravity.empty())        // (only with the extensions, so the reference's log stays as it is)
        prob.on_adapt = [&](int step, int64_t before, int64_t after) {     // the choice is made again on every adapted mesh
          if (!gravity.empty()) { std::cout << "adapted before step " << step << ": "; gravity_line(std::cout); std::cout << std::endl; }
          if (!tensor_top.empty()) { std::cout << "adapted before step " << step << ": "; tensor_line(std::cout); std::cout << std::endl; }
          if (!moduli_top.empty()) { std::cout << "adapted before step " << step << ": "; moduli_line(std::cout); std::cout << std::endl; }
          std::cout << "adapted before step " << step << ": " << before << " -> " << after << " cells; prescribed pressures: " << prob.problem()->d.n_dirichlet_p
                    << " dofs; pressure preconditioner: " << prec_name[prob.pressure_solver.control.preconditioner] << ", projection preconditioner: "
                    << prec_name[prob.strain_projector.control.preconditioner] << std::endl;
        };
      prob.flow_controls.flow_balance = flow_balance; prob.flow_controls.darcy_output = darcy_output;
      prob.stress_controls.stress_output = stress_output; prob.stress_controls.force_balance = force_balance; prob.stress_controls.failure_log = mohr_coulomb;
      prob.stress_controls.mohr_coulomb = mohr_coulomb; prob.stress_controls.cohesion = mc_cohesion; prob.stress_controls.friction_angle = mc_friction_deg * 3.14159265358979323846 / 180.0;
      rows = prob.run(rc, trace.data(), (int)trace.size() / 8);
      if (force_balance) {               // (only with the option)
        char buf[256];
        const int dm = prob.problem()->d.dim; const double sqrt_n = std::sqrt((double)prob.problem()->d.n_dofs_u);
        for (size_t s = 0; s < prob.force_history.size(); ++s) {
          const auto &B = prob.force_history[s]; const poro_force_balance_terms &t = B.terms;
          std::snprintf(buf, sizeof buf, "force balance step %zu:", s + 1);
          std::string line = buf;
          for (size_t k = 0; k < B.labels.size(); ++k) { std::snprintf(buf, sizeof buf, " label %d component %d reaction %.9e;", (int)B.labels[k], (int)B.components[k], B.reaction_by_label[k]); line += buf; }
          for (int k = 0; k < dm; ++k) {
            std::snprintf(buf, sizeof buf, " component %d: reaction %.9e traction %.9e body %.9e coupling %.3e free_rows %.3e closure %.3e bound %.3e;", k, t.reaction_sum[k], t.traction_sum[k], t.body_sum[k],
                          t.coupling_sum[k], t.free_row_sum[k], B.imbalance(k), sqrt_n * t.residual_l2);
            line += buf;
          }
          std::snprintf(buf, sizeof buf, " residual_l2 %.9e", t.residual_l2); line += buf;
          force_lines.push_back(line);
        }
      }
      if (mohr_coulomb) {
        char buf[256];
        for (size_t s = 0; s < prob.failure_history.size(); ++s) {
          const poro_failure_summary &f = prob.failure_history[s];
          std::snprintf(buf, sizeof buf, "mohr-coulomb step %zu: max f %.9e in cell %lld, %lld failing cells", s + 1, f.max_f, (long long)f.argmax_cell, (long long)f.n_failing);
          failure_lines.push_back(buf);
        }
      }
      if (flow_balance) {                // (only with the option) the per-step lines, printed with the steps below, and the totals
        char buf[256];
        const double sqrt_n = std::sqrt((double)prob.problem()->d.n_dofs_p);
        for (size_t s = 0; s < prob.flow_history.size(); ++s) {
          const auto &B = prob.flow_history[s]; const poro_flow_balance_terms &t = B.terms;
          std::snprintf(buf, sizeof buf, "flow balance step %zu: storage_strain %.9e storage_pressure %.9e source %.9e outflow %.9e free_rows %.9e residual_l2 %.9e;", s + 1,
                        t.storage_rate_strain, t.storage_rate_pressure, t.source_sum, t.outflow_prescribed, t.free_row_sum, t.residual_l2);
          std::string line = buf;
          for (size_t k = 0; k < B.labels.size(); ++k) { std::snprintf(buf, sizeof buf, " label %d outflow %.9e discharge %.9e;", (int)B.labels[k], B.outflow_by_label[k], B.discharge_by_label[k]); line += buf; }
          std::snprintf(buf, sizeof buf, " imbalance %.3e bound %.3e", B.imbalance(), sqrt_n * t.residual_l2); line += buf;
          flow_lines.push_back(line);
        }
        const auto &T = prob.flow_totals;
        std::snprintf(buf, sizeof buf, "flow balance totals over %d steps: storage_strain %.9e storage_pressure %.9e injected %.9e drained %.9e;", T.steps, T.storage_strain, T.storage_pressure, -T.source, T.outflow);
        std::string line = buf;
        for (size_t k = 0; k < T.labels.size(); ++k) { std::snprintf(buf, sizeof buf, " label %d drained %.9e face-integrated %.9e;", (int)T.labels[k], T.outflow_by_label[k], T.discharge_by_label[k]); line += buf; }
        std::snprintf(buf, sizeof buf, " imbalance %.3e bound %.3e", T.storage_strain + T.storage_pressure + T.source + T.outflow, T.bound); line += buf;
        flow_lines.push_back(line);
      }
      if (rc.fdm_per_direction) {           // (only with the option, so the reference's log stays as it is)
        static const char *const runs[] = {"nodal kernels", "octant form", "per-direction form", "slab form", "planar form"};
        int32_t req = 0, eff = 0, split[3] = {0, 0, 0};
        if (poro_ctx_get_fdm_form(prob.context(), &req, &eff, split) != 0) throw std::runtime_error(poro_last_error());
        std::cout << "block FDM form: " << runs[eff] << ", split directions (x y z): " << split[0] << " " << split[1] << " " << split[2] << std::endl;
      }
      if (!moduli_top.empty()) { moduli_line(std::cout); std::cout << std::endl; }
      if (!gravity.empty()) { gravity_line(std::cout); std::cout << std::endl; }
      if (!tensor_top.empty()) { tensor_line(std::cout); std::cout << std::endl; }
      if (!layer_top.empty()) {
        int32_t kind = 0;
        if (poro_ctx_get_cell_permeability(prob.context(), nullptr, 0, &kind) != 0) throw std::runtime_error(poro_last_error());
        std::cout << "permeability layers: " << layer_top.size() << ", field kind " << kind << "; pressure preconditioner: " << prec_name[prob.pressure_solver.control.preconditioner] << std::endl;
      }
      if (!pressure_labels.empty())
        std::cout << "prescribed pressures: " << prob.problem()->d.n_dirichlet_p << " dofs; pressure preconditioner: " << prec_name[prob.pressure_solver.control.preconditioner]
                  << ", projection preconditioner: " << prec_name[prob.strain_projector.control.preconditioner] << std::endl;
    };
    if (data.dim == 2) { PoroElasticProblem<2> prob(P, device, op); go(prob); }
    else { PoroElasticProblem<3> prob(P, device, op); go(prob); }
    for (int r = 1; r < rows; ++r) {
      const double *t = &trace[8 * r];
      if (t[1] == 1) std::cout << "Time: " << t[0] * rc.time_step << std::endl;                  // :330
      std::cout << "    Coupling iteration: " << (int)t[1] << std::endl;                         // :352
      std::cout << "        pressure converged; iterations: " << (int)t[2] << std::endl;        // :367-369
      std::cout << "Solution limits: " << t[4] << "\t" << std::endl;                             // :387-389
      std::cout << "        Error: " << t[5] << std::endl;                                       // :406
      const size_t step = (size_t)t[0];           // --flow-balance: the step's line behind its last coupling iteration
      if (step >= 1 && step + 1 <= flow_lines.size() && (r + 1 == rows || trace[8 * (r + 1)] != t[0])) std::cout << flow_lines[step - 1] << std::endl;
      if (step >= 1 && (r + 1 == rows || trace[8 * (r + 1)] != t[0])) {     // --force-balance, --mohr-coulomb: the step's lines behind its last coupling iteration
        if (step <= force_lines.size()) std::cout << force_lines[step - 1] << std::endl;
        if (step <= failure_lines.size()) std::cout << failure_lines[step - 1] << std::endl;
      }
    }
    if (!flow_lines.empty()) std::cout << flow_lines.back() << std::endl;
  } catch (std::exception &exc) {   // PoroelasticityFSS.h:512-523
    std::cerr << std::endl << "----------------------------------------------------" << std::endl
              << "Exception on processing: " << std::endl << exc.what() << std::endl << "Aborting!" << std::endl
              << "----------------------------------------------------" << std::endl;
    return 1;
  }
  return 0;
}
