// C entry points of the host layer (mesh / DoF / FE-table provider, parameter file front end and the
// run() driver), so tests and bench.py can reach the C++ host code through ctypes.
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include "input_data.hpp"
#include "mesh.hpp"
#include "problem.hpp"
#include "../csrc/kelly_tables.hpp"

using namespace poro_host;

namespace {
thread_local std::string g_err;
void fill_bc(BoundaryConditions &bc, int n_dir, const int32_t *dl, const int32_t *dc, const double *dv,
             int n_neu, const int32_t *nl, const int32_t *nc, const double *nv) {
  bc.dirichlet_labels.assign(dl, dl + n_dir); bc.dirichlet_components.assign(dc, dc + n_dir); bc.dirichlet_values.assign(dv, dv + n_dir);
  bc.neumann_labels.assign(nl, nl + n_neu); bc.neumann_components.assign(nc, nc + n_neu); bc.neumann_values.assign(nv, nv + n_neu);
}
// f(problem behind the handle): 0, or -1 with what it threw in poro_host_last_error()
template <class F> int on_problem(void *h, F &&f) {
  try { f(*static_cast<ProblemData *>(h)); return 0; }
  catch (const std::exception &e) { g_err = e.what(); return -1; }
}
// an array of a per-cell field the problem carries: its length (0: none); copied where out != NULL
int64_t copy_field(const std::vector<double> &f, double *out) {
  if (out && !f.empty()) std::memcpy(out, f.data(), f.size() * sizeof(double));
  return (int64_t)f.size();
}
// component a of a field (none where the field has fewer)
int64_t copy_field(const ProblemData::PerCellField &f, int a, double *out) { return a < f.ncomp() ? copy_field(f.comp[a], out) : 0; }
// what poro_host_runner_create hands out: the problem of either dimension and the options it runs with
struct HostRunner {
  int dim; RunControls rc; PoroElasticProblem<2> *p2 = nullptr; PoroElasticProblem<3> *p3 = nullptr;
  ~HostRunner() { delete p2; delete p3; }
};
// f(the PoroElasticProblem<dim> the runner holds, its RunControls)
template <class F> auto on_runner(void *r, F &&f) {
  auto *R = static_cast<HostRunner *>(r);
  if (R->dim == 2) return f(*R->p2, R->rc);
  return f(*R->p3, R->rc);
}
// the same for the calls that report 0 / -1
template <class F> int try_on_runner(void *r, F &&f) {
  try { on_runner(r, f); return 0; }
  catch (const std::exception &e) { g_err = e.what(); return -1; }
}
// work[11] = apply_u, apply_p, asm_rhs_u, asm_matrix_u, residual_p, jacobian_p, proj_rhs, cg_u, cg_p, cg_proj, seconds_solve_u*1e6
template <class W> void fill_work(const W &w, int64_t *work) {
  const int64_t all[11] = {w.apply_u, w.apply_p, w.asm_rhs_u, w.asm_matrix_u, w.residual_p, w.jacobian_p, w.proj_rhs, w.cg_u, w.cg_p, w.cg_proj, (int64_t)(w.seconds_solve_u * 1e6)};
  std::copy(all, all + 11, work);
}
}  // namespace

extern "C" {

const char *poro_host_last_error() { return g_err.c_str(); }

// structured box (or one slab of it): GridGenerator::hyper_rectangle(colorize) + uniform refinement
void *poro_host_build_box(int dim, const int32_t *n, const double *size, int k_u, int rank, int n_ranks,
                          int n_dir, const int32_t *dl, const int32_t *dc, const double *dv,
                          int n_neu, const int32_t *nl, const int32_t *nc, const double *nv, const poro_material *mat) {
  try {
    auto *P = new ProblemData();
    fill_bc(P->bc, n_dir, dl, dc, dv, n_neu, nl, nc, nv);
    P->mat = *mat;
    int nn[3] = {n[0], n[1], dim == 3 ? n[2] : 1}; double sz[3] = {size[0], size[1], dim == 3 ? size[2] : 1};
    build_box_problem(*P, dim, nn, sz, k_u, rank, n_ranks);
    return P;
  } catch (const std::exception &e) { g_err = e.what(); return nullptr; }
}

// graded box (no box tag: general kernels), see build_graded_box_problem
void *poro_host_build_graded_box(int dim, const int32_t *n, const double *size, int k_u, const double *grading,
                                 int n_dir, const int32_t *dl, const int32_t *dc, const double *dv,
                                 int n_neu, const int32_t *nl, const int32_t *nc, const double *nv, const poro_material *mat) {
  try {
    auto *P = new ProblemData();
    fill_bc(P->bc, n_dir, dl, dc, dv, n_neu, nl, nc, nv);
    P->mat = *mat;
    int nn[3] = {n[0], n[1], dim == 3 ? n[2] : 1}; double sz[3] = {size[0], size[1], dim == 3 ? size[2] : 1}, gr[3] = {grading[0], grading[1], dim == 3 ? grading[2] : 0.0};
    build_graded_box_problem(*P, dim, nn, sz, k_u, gr);
    return P;
  } catch (const std::exception &e) { g_err = e.what(); return nullptr; }
}

// box with one locally refined block of cells (hanging nodes): the mesh class one refine_mesh() pass produces (PoroelasticityFSS.h:447-498)
void *poro_host_build_refined_box(int dim, const int32_t *n, const double *size, int k_u, const int32_t *lo, const int32_t *hi,
                                  int n_dir, const int32_t *dl, const int32_t *dc, const double *dv,
                                  int n_neu, const int32_t *nl, const int32_t *nc, const double *nv, const poro_material *mat) {
  try {
    auto *P = new ProblemData();
    fill_bc(P->bc, n_dir, dl, dc, dv, n_neu, nl, nc, nv);
    P->mat = *mat;
    int nn[3] = {n[0], n[1], dim == 3 ? n[2] : 1}; double sz[3] = {size[0], size[1], dim == 3 ? size[2] : 1};
    int l3[3] = {lo[0], lo[1], dim == 3 ? lo[2] : 0}, h3[3] = {hi[0], hi[1], dim == 3 ? hi[2] : 1};
    build_refined_box_problem(*P, dim, nn, sz, k_u, l3, h3);
    return P;
  } catch (const std::exception &e) { g_err = e.what(); return nullptr; }
}

// the same mesh class from a mask: mask[c] != 0 = coarse cell c (lexicographic, x fastest) is split once.  The block form above is this with the block's mask (same
// numbering).  An all-zero mask gives the uniform box as a GENERAL mesh with the coarse space and no box tag (the starting point of an adaptive run); the structured
// kernels need poro_host_build_box.
void *poro_host_build_refined_box_mask(int dim, const int32_t *n, const double *size, int k_u, const int32_t *mask,
                                       int n_dir, const int32_t *dl, const int32_t *dc, const double *dv,
                                       int n_neu, const int32_t *nl, const int32_t *nc, const double *nv, const poro_material *mat) {
  try {
    std::unique_ptr<ProblemData> P(new ProblemData());
    fill_bc(P->bc, n_dir, dl, dc, dv, n_neu, nl, nc, nv);
    P->mat = *mat;
    int nn[3] = {n[0], n[1], dim == 3 ? n[2] : 1}; double sz[3] = {size[0], size[1], dim == 3 ? size[2] : 1};
    if (nn[0] < 1 || nn[1] < 1 || nn[2] < 1) throw std::runtime_error("refined_box_mask: n must be positive");
    std::vector<uint8_t> m((size_t)nn[0] * nn[1] * nn[2]);
    for (size_t i = 0; i < m.size(); ++i) m[i] = mask[i] ? 1 : 0;
    build_refined_box_problem_mask(*P, dim, nn, sz, k_u, m);
    return P.release();
  } catch (const std::exception &e) { g_err = e.what(); return nullptr; }
}
// what a refined box keeps for adaptation.  Both return the length (n_coarse_cells / n_cells), or -1 when the problem is no refined box; they copy when the pointers are given
int64_t poro_host_refine_mask(void *h, int32_t *mask) {
  auto *P = static_cast<ProblemData *>(h);
  if (!P->refined_box) { g_err = "not a mask- or block-refined box"; return -1; }
  if (mask) for (size_t i = 0; i < P->refine_mask.size(); ++i) mask[i] = P->refine_mask[i];
  return (int64_t)P->refine_mask.size();
}
// per cell of the mesh: its coarse cell and its child number (cx + 2 cy + 4 cz; -1 = the coarse cell itself)
int64_t poro_host_cell_parents(void *h, int32_t *coarse, int32_t *child) {
  auto *P = static_cast<ProblemData *>(h);
  if (!P->refined_box) { g_err = "not a mask- or block-refined box"; return -1; }
  if (coarse) std::memcpy(coarse, P->cell_coarse.data(), P->cell_coarse.size() * sizeof(int32_t));
  if (child) std::memcpy(child, P->cell_child.data(), P->cell_child.size() * sizeof(int32_t));
  return (int64_t)P->cell_coarse.size();
}
// refine_and_coarsen_fixed_fraction + the level limits of refine_mesh (PoroelasticityFSS.h:460-472) as the mask of the next mesh; the rule is stated at mark_fixed_fraction (mesh.hpp)
int poro_host_mark_fixed_fraction(void *h, const double *eta /* [n_cells] */, double refine_fraction, double coarsen_fraction, int32_t *new_mask /* [n_coarse_cells] */) {
  try {
    std::vector<uint8_t> m;
    mark_fixed_fraction(*static_cast<ProblemData *>(h), eta, refine_fraction, coarsen_fraction, m);
    for (size_t i = 0; i < m.size(); ++i) new_mask[i] = m[i];
    return 0;
  } catch (const std::exception &e) { g_err = e.what(); return -1; }
}
// SolutionTransfer::interpolate (:474-497) for the pressure space as rows: new dof i = sum weight * old dof node (see transfer_rows_p, mesh.hpp).  Two calls as for
// poro_host_local_to_global: with node == NULL it fills ptr[n_new + 1] (when given) and returns the entry count, with node / weight it fills those too.  < 0: error
int64_t poro_host_transfer_rows_p(void *old_problem, void *new_problem, int64_t *ptr, int32_t *node, double *weight) {
  try {
    std::vector<int64_t> p; std::vector<int32_t> nd; std::vector<double> w;
    transfer_rows_p(*static_cast<ProblemData *>(old_problem), *static_cast<ProblemData *>(new_problem), p, nd, w);
    if (ptr) std::memcpy(ptr, p.data(), p.size() * sizeof(int64_t));
    if (node) std::memcpy(node, nd.data(), nd.size() * sizeof(int32_t));
    if (weight) std::memcpy(weight, w.data(), w.size() * sizeof(double));
    return (int64_t)nd.size();
  } catch (const std::exception &e) { g_err = e.what(); return -1; }
}

// the face tables poro_pres_estimate_error builds for this problem's descriptor (csrc/kelly_tables.hpp; the same code, run on the descriptor's host arrays), so that
// they can be checked without a GPU.  Returns the face count and *n_entries (< 0: error); fills the arrays that are given: per face cell_a / cell_b / code, per cell
// ent_ptr[n_cells + 1], per entry ent_face / ent_hcell
int64_t poro_host_kelly_tables(void *h, int64_t *n_entries, int32_t *cell_a, int32_t *cell_b, int32_t *code, int64_t *ent_ptr, int32_t *ent_face, int32_t *ent_hcell) {
  try {
    const poro_desc &d = static_cast<ProblemData *>(h)->d;
    const int nv = 1 << d.dim; const poro_constraints &c = d.cons_p; const int64_t nm = c.n ? c.ptr[c.n] : 0;
    const poro::KellyTables T = poro::build_kelly_tables_host(d.dim, d.n_cells, d.n_dofs_p, std::vector<int32_t>(d.cell_dofs_p, d.cell_dofs_p + d.n_cells * nv), d.n_bfaces,
        std::vector<int32_t>(d.bface_cell, d.bface_cell + d.n_bfaces), std::vector<int32_t>(d.bface_local, d.bface_local + d.n_bfaces), c.n,
        std::vector<int32_t>(c.dof, c.dof + c.n), c.n ? std::vector<int64_t>(c.ptr, c.ptr + c.n + 1) : std::vector<int64_t>(1, 0), std::vector<int32_t>(c.master, c.master + nm),
        std::vector<double>(c.weight, c.weight + nm));
    auto put = [](auto *dst, const auto &src) { if (dst) std::copy(src.begin(), src.end(), dst); };
    put(cell_a, T.cell_a); put(cell_b, T.cell_b); put(code, T.code); put(ent_ptr, T.ent_ptr); put(ent_face, T.ent_face); put(ent_hcell, T.ent_hcell);
    if (n_entries) *n_entries = (int64_t)T.ent_face.size();
    return (int64_t)T.cell_a.size();
  } catch (const std::exception &e) { g_err = e.what(); return -1; }
}

// Gmsh 2.2 mesh (GridIn::read_msh, PoroelasticityFSS.h:438-445)
void *poro_host_build_gmsh(const char *path, int k_u,
                           int n_dir, const int32_t *dl, const int32_t *dc, const double *dv,
                           int n_neu, const int32_t *nl, const int32_t *nc, const double *nv, const poro_material *mat) {
  try {
    auto *P = new ProblemData();
    fill_bc(P->bc, n_dir, dl, dc, dv, n_neu, nl, nc, nv);
    P->mat = *mat;
    P->mesh = read_gmsh22(path);
    P->finalize(k_u);
    attach_auxiliary_box(*P, k_u);     // (where the mesh fills a rectangle with colorized side ids: coarse space of the two-level preconditioner)
    return P;
  } catch (const std::exception &e) { g_err = e.what(); return nullptr; }
}
// the same mesh after `refine` uniform refinements (refine_global of read_mesh()'s grid)
void *poro_host_build_gmsh_refined(const char *path, int k_u, int refine,
                                   int n_dir, const int32_t *dl, const int32_t *dc, const double *dv,
                                   int n_neu, const int32_t *nl, const int32_t *nc, const double *nv, const poro_material *mat) {
  try {
    auto *P = new ProblemData();
    fill_bc(P->bc, n_dir, dl, dc, dv, n_neu, nl, nc, nv);
    P->mat = *mat;
    P->mesh = read_gmsh22(path);
    for (int r = 0; r < refine; ++r) P->mesh = refine_quads(P->mesh);
    P->finalize(k_u);
    attach_auxiliary_box(*P, k_u);
    return P;
  } catch (const std::exception &e) { g_err = e.what(); return nullptr; }
}

// piece `rank` of a general n_ranks partition of a global problem (Morton cell ranges + interface lists); the global problem stays valid
void *poro_host_partition(void *global, int rank, int n_ranks) {
  try { auto *L = new ProblemData(); try { partition_problem(*static_cast<ProblemData *>(global), rank, n_ranks, *L); } catch (...) { delete L; throw; } return L; }
  catch (const std::exception &e) { g_err = e.what(); return nullptr; }
}
// the same with options.  flags = 1: the piece carries the coarse space of the two-level preconditioner (its own copy of the global box problem + the global
// interpolation rows of its nodes; displacement ghosts and owners per node).  Refused when the global problem has no coarse space
void *poro_host_partition_ex(void *global, int rank, int n_ranks, int flags) {
  try { auto *L = new ProblemData(); try { partition_problem(*static_cast<ProblemData *>(global), rank, n_ranks, *L, (flags & 1) != 0); } catch (...) { delete L; throw; } return L; }
  catch (const std::exception &e) { g_err = e.what(); return nullptr; }
}
// local -> global dof map of a piece (space 0: displacement, 1: pressure); returns the length, copies when out != NULL
int64_t poro_host_local_to_global(void *h, int space, int32_t *out) {
  auto &v = space == 0 ? static_cast<ProblemData *>(h)->local_to_global_u : static_cast<ProblemData *>(h)->local_to_global_p;
  if (out) std::memcpy(out, v.data(), v.size() * sizeof(int32_t));
  return (int64_t)v.size();
}

// extension: prescribed pressures on boundary labels (before the context is created)
int poro_host_set_pressure_bc(void *h, int n, const int32_t *labels, const double *values) {
  try {
    auto *P = static_cast<ProblemData *>(h);
    P->bc.pressure_labels.assign(labels, labels + n); P->bc.pressure_values.assign(values, values + n);
    P->set_pressure_bc();
    return 0;
  } catch (const std::exception &e) { g_err = e.what(); return -1; }
}
// per entry of poro_desc.dirichlet_dof_p the boundary label that prescribed it (first condition in list order on shared edges); returns the length, copies when out != NULL
int64_t poro_host_pressure_bc_labels(void *h, int32_t *out) {
  const auto &v = static_cast<ProblemData *>(h)->dirichlet_label_p;
  if (out && !v.empty()) std::memcpy(out, v.data(), v.size() * sizeof(int32_t));
  return (int64_t)v.size();
}
// per entry of poro_desc.dirichlet_dof the (boundary label, component) of the displacement condition that prescribed it (first condition in list order), two entries per
// dof; returns the number of dofs, copies when out != NULL.  0 where the list was given by the caller (pieces of a partition)
int64_t poro_host_displacement_bc_labels(void *h, int32_t *out) {
  const auto &v = static_cast<ProblemData *>(h)->dirichlet_label_u;
  if (out && !v.empty()) std::memcpy(out, v.data(), v.size() * sizeof(int32_t));
  return (int64_t)(v.size() / 2);
}
// extension: rigid frictionless plates - component `components[i]` of the displacement takes ONE (unknown) value on the boundary `labels[i]` (before the context is created)
int poro_host_tie_boundary(void *h, int n, const int32_t *labels, const int32_t *components) {
  try {
    auto *P = static_cast<ProblemData *>(h);
    if (P->part.n_ranks > 1) throw std::runtime_error("tie_boundary: implemented for one rank");
    if (P->ties_added) throw std::runtime_error("tie_boundary: already applied");
    P->bc.tie_labels.assign(labels, labels + n); P->bc.tie_components.assign(components, components + n);
    for (int i = 0; i < n; ++i) if (components[i] < 0 || components[i] >= P->mesh.dim) throw std::runtime_error("tie_boundary: component out of range");
    P->finalize(P->dofs.k_u, true);
    return 0;
  } catch (const std::exception &e) { g_err = e.what(); return -1; }
}
// extension: per-cell k / mu of the pressure system, one value per cell of the problem's mesh (values == NULL: back to the scalar).  Kept with the problem; the drivers
// hand it to every context they create from it (poro_ctx_set_cell_permeability), also on the meshes an adaptive run builds (a child takes its parent's value)
int poro_host_set_cell_permeability(void *h, const double *values, int64_t n) { return on_problem(h, [&](ProblemData &P) { P.set_cell_permeability(values, n); }); }
// the same by layers of the slowest direction: a cell takes the first layer whose top[l] is >= the coordinate of its centre
int poro_host_set_permeability_layers(void *h, int n, const double *top, const double *value) { return on_problem(h, [&](ProblemData &P) { P.set_permeability_layers(n, top, value); }); }
// what refine_mesh does with the field: `h` (a refined box) takes the field of `old` (a refined box over the same coarse box), cell by coarse cell
int poro_host_inherit_cell_permeability(void *h, void *old) { return on_problem(h, [&](ProblemData &P) { P.inherit_cell_permeability(*static_cast<ProblemData *>(old)); }); }
// the field the problem carries: returns its length (0: none), copies when out != NULL
int64_t poro_host_get_cell_permeability(void *h, double *out) { const ProblemData &P = *static_cast<ProblemData *>(h); return P.carries_permeability(false) ? copy_field(P.permeability, 0, out) : 0; }
// extension: the per-cell diagonal tensor diag(kx, ky[, kz]) / mu, values[n][dim] with x first (NULL: none); a problem carries the scalar field or the tensor
int poro_host_set_cell_permeability_tensor(void *h, const double *values, int64_t n) { return on_problem(h, [&](ProblemData &P) { P.set_cell_permeability_tensor(values, n); }); }
int poro_host_set_permeability_tensor_layers(void *h, int n, const double *top, const double *kx, const double *ky, const double *kz /* not read in 2D */) { return on_problem(h, [&](ProblemData &P) { P.set_permeability_tensor_layers(n, top, kx, ky, kz); }); }
int poro_host_inherit_cell_permeability_tensor(void *h, void *old) { return on_problem(h, [&](ProblemData &P) { P.inherit_cell_permeability_tensor(*static_cast<ProblemData *>(old)); }); }
// returns the number of doubles the problem carries (n_cells * dim; 0: none), out[cell][dim]
int64_t poro_host_get_cell_permeability_tensor(void *h, double *out) { const ProblemData &P = *static_cast<ProblemData *>(h); return P.carries_permeability(true) ? copy_field(P.permeability.interleaved(), out) : 0; }
// extension: per-cell Lame lambda and shear modulus G of the displacement system (both NULL: back to the scalars); kept with the problem and handed over like the permeability
int poro_host_set_cell_moduli(void *h, const double *lam, const double *G, int64_t n) { return on_problem(h, [&](ProblemData &P) { P.set_cell_moduli(lam, G, n); }); }
// by layers of the slowest direction: a cell takes the first layer whose top[l] is >= the coordinate of its centre; (E, nu) -> (lambda, G) as the parameter file's are
int poro_host_set_moduli_layers(void *h, int n, const double *top, const double *young, const double *poisson) { return on_problem(h, [&](ProblemData &P) { P.set_moduli_layers(n, top, young, poisson); }); }
int poro_host_inherit_cell_moduli(void *h, void *old) { return on_problem(h, [&](ProblemData &P) { P.inherit_cell_moduli(*static_cast<ProblemData *>(old)); }); }
// the field the problem carries: returns its length (0: none), copies where the pointers are not NULL
int64_t poro_host_get_cell_moduli(void *h, double *lam_out, double *G_out) {
  const ProblemData &P = *static_cast<ProblemData *>(h); copy_field(P.moduli, 1, G_out);
  return copy_field(P.moduli, 0, lam_out);
}
// extension: gravity.  g[dim] (NULL or zeros: off), the fluid density of the Darcy gravity flux (0: none), the scalar bulk density (< 0: keep the present one, 2700 at
// first) and whether a run starts from the hydrostatic pressure; kept with the problem, handed to every context the drivers create (poro_ctx_set_gravity)
int poro_host_set_gravity(void *h, const double *g, double fluid_density, double bulk_density, int hydrostatic_init) {
  return on_problem(h, [&](ProblemData &P) { P.set_gravity(g, fluid_density, bulk_density); P.hydrostatic_init = hydrostatic_init != 0; });
}
// what the problem carries: g[3], the two scalar densities, the hydrostatic start; returns 1 while some component of g is not zero
int poro_host_get_gravity(void *h, double *g, double *fluid_density, double *bulk_density, int32_t *hydrostatic_init) {
  const ProblemData &P = *static_cast<ProblemData *>(h);
  for (int d = 0; g && d < 3; ++d) g[d] = P.gravity[d];
  if (fluid_density) *fluid_density = P.fluid_density;
  if (bulk_density) *bulk_density = P.bulk_density;
  if (hydrostatic_init) *hydrostatic_init = P.hydrostatic_init ? 1 : 0;
  return P.has_gravity() ? 1 : 0;
}
// per-cell bulk density (values == NULL: back to the scalar), by layers of the slowest direction, through a refine / coarsen pair, and what the problem carries
int poro_host_set_cell_density(void *h, const double *values, int64_t n) { return on_problem(h, [&](ProblemData &P) { P.set_cell_density(values, n); }); }
int poro_host_set_density_layers(void *h, int n, const double *top, const double *rho) { return on_problem(h, [&](ProblemData &P) { P.set_density_layers(n, top, rho); }); }
int poro_host_inherit_cell_density(void *h, void *old) { return on_problem(h, [&](ProblemData &P) { P.inherit_cell_density(*static_cast<ProblemData *>(old)); }); }
int64_t poro_host_get_cell_density(void *h, double *out) { return copy_field(static_cast<ProblemData *>(h)->density, 0, out); }
const poro_desc *poro_host_desc(void *h) { return &static_cast<ProblemData *>(h)->d; }
void poro_host_free(void *h) { delete static_cast<ProblemData *>(h); }

// InputDataPoroel::read_input_file flattened for ctypes
typedef struct poro_input_flat {
  int32_t dim; double domain_size[3]; int32_t initial_refinement_level, max_refinement_level;
  double youngs_modulus, poisson_ratio, biot_coef, perm, poro, visc, bulk_density, f_comp, r_well, flow_rate;
  double p_init, time_step, t_max, fss_tol, pressure_tol; int32_t max_fss_iterations, max_pressure_iterations;
  int32_t n_dirichlet, dirichlet_labels[16], dirichlet_components[16]; double dirichlet_values[16];
  int32_t n_neumann, neumann_labels[16], neumann_components[16]; double neumann_values[16];
  double lame_constant, shear_modulus, bulk_modulus, grain_bulk_modulus, n_modulus, m_modulus;
  poro_material material;
} poro_input_flat;

int poro_host_read_input(const char *path /* NULL = declared defaults */, poro_input_flat *o) {
  try {
    input_data::InputDataPoroel in;
    if (path) in.read_input_file(path);
    std::memset(o, 0, sizeof(*o));
    o->dim = in.dim;
    for (size_t i = 0; i < in.domain_size.size() && i < 3; ++i) o->domain_size[i] = in.domain_size[i];
    o->initial_refinement_level = in.initial_refinement_level; o->max_refinement_level = in.max_refinement_level;
    o->youngs_modulus = in.youngs_modulus; o->poisson_ratio = in.poisson_ratio; o->biot_coef = in.biot_coef; o->perm = in.perm; o->poro = in.poro;
    o->visc = in.visc; o->bulk_density = in.bulk_density; o->f_comp = in.f_comp; o->r_well = in.r_well; o->flow_rate = in.flow_rate;
    o->p_init = in.p_init; o->time_step = in.time_step; o->t_max = in.t_max; o->fss_tol = in.fss_tol; o->pressure_tol = in.pressure_tol;
    o->max_fss_iterations = in.max_fss_iterations; o->max_pressure_iterations = in.max_pressure_iterations;
    if (in.displacement_boundary_labels.size() > 16 || in.stress_boundary_labels.size() > 16) throw std::runtime_error("more than 16 boundary conditions");
    if (in.displacement_boundary_labels.size() != in.displacement_boundary_components.size() || in.displacement_boundary_labels.size() != in.displacement_boundary_values.size() ||
        in.stress_boundary_labels.size() != in.stress_boundary_components.size() || in.stress_boundary_labels.size() != in.stress_boundary_values.size())
      throw std::runtime_error("boundary label / component / value lists differ in length");
    o->n_dirichlet = (int32_t)in.displacement_boundary_labels.size();
    for (int i = 0; i < o->n_dirichlet; ++i) { o->dirichlet_labels[i] = in.displacement_boundary_labels[i]; o->dirichlet_components[i] = in.displacement_boundary_components[i]; o->dirichlet_values[i] = in.displacement_boundary_values[i]; }
    o->n_neumann = (int32_t)in.stress_boundary_labels.size();
    for (int i = 0; i < o->n_neumann; ++i) { o->neumann_labels[i] = in.stress_boundary_labels[i]; o->neumann_components[i] = in.stress_boundary_components[i]; o->neumann_values[i] = in.stress_boundary_values[i]; }
    o->lame_constant = in.lame_constant; o->shear_modulus = in.shear_modulus; o->bulk_modulus = in.bulk_modulus;
    o->grain_bulk_modulus = in.grain_bulk_modulus; o->n_modulus = in.n_modulus; o->m_modulus = in.m_modulus;
    o->material = in.material();
    return 0;
  } catch (const std::exception &e) { g_err = e.what(); return -1; }
}

// PoroElasticProblem<dim>::run() on the HIP back end (problem.hpp); the options: host/run_controls.hpp.  trace rows: see PoroElasticProblem::time_step.
// With mesh adaptation (opts->refine_every > 0: refine_mesh every refine_every-th step, PoroelasticityFSS.h:333-340) the problem must be a mask- or block-refined box, and
// *problem_out receives the mesh the run ended on when it was refined at least once (the caller frees it with poro_host_free; the context in *ctx_out belongs to it),
// else NULL (the context belongs to `problem_data`).
int poro_host_run_adaptive(void *problem_data, int device, int operator_mode, const poro_host_run_options *opts, double *trace, int max_rows, poro_ctx **ctx_out, void **problem_out) {
  try {
    auto *P = static_cast<ProblemData *>(problem_data);
    const RunControls rc = to_run_controls(*opts);
    if (rc.refine_every > 0 && !problem_out) throw std::runtime_error("run: refine_every needs poro_host_run_adaptive, which hands out the mesh the run ends on");
    int rows = 0;
    if (problem_out) *problem_out = nullptr;
    auto go = [&](auto &&prob) { rows = prob.run(rc, trace, max_rows); if (problem_out) *problem_out = prob.release_problem(); if (ctx_out) *ctx_out = prob.release(); };
    if (P->mesh.dim == 2) go(PoroElasticProblem<2>(*P, device, operator_mode)); else go(PoroElasticProblem<3>(*P, device, operator_mode));
    return rows;
  } catch (const std::exception &e) { g_err = e.what(); return -1; }
}
// the same on one mesh (refine_every must be 0)
int poro_host_run(void *problem_data, int device, int operator_mode, const poro_host_run_options *opts, double *trace, int max_rows, poro_ctx **ctx_out) {
  return poro_host_run_adaptive(problem_data, device, operator_mode, opts, trace, max_rows, ctx_out, nullptr);
}

// Steppable driver for bench.py (HostRunner): the same PoroElasticProblem object, one time step per call.
void *poro_host_runner_create(void *problem_data, int device, int operator_mode, const poro_host_run_options *opts) {
  try {
    auto *P = static_cast<ProblemData *>(problem_data);
    std::unique_ptr<HostRunner> R(new HostRunner()); R->dim = P->mesh.dim; R->rc = to_run_controls(*opts);
    if (R->dim == 2) R->p2 = new PoroElasticProblem<2>(*P, device, operator_mode); else R->p3 = new PoroElasticProblem<3>(*P, device, operator_mode);
    return R.release();
  } catch (const std::exception &e) { g_err = e.what(); return nullptr; }
}
// refine_mesh + the two calls of PoroelasticityFSS.h:338-339 between two steps; cells[2] = cell counts before and after.  Afterwards poro_host_runner_ctx and
// poro_host_runner_problem give the new context and mesh, both owned (and freed) by the runner
int poro_host_runner_adapt(void *r, double refine_fraction, double coarsen_fraction, int64_t *cells) {
  return try_on_runner(r, [&](auto &prob, RunControls rc) {
    rc.refine_fraction = refine_fraction; rc.coarsen_fraction = coarsen_fraction;
    const std::pair<int64_t, int64_t> n = prob.refine_mesh(rc);
    if (cells) { cells[0] = n.first; cells[1] = n.second; }
  });
}
void *poro_host_runner_problem(void *r) { return on_runner(r, [](auto &prob, const RunControls &) { return const_cast<ProblemData *>(prob.problem()); }); }
poro_ctx *poro_host_runner_ctx(void *r) { return on_runner(r, [](auto &prob, const RunControls &) { return prob.context(); }); }
int poro_host_runner_initialize(void *r) { return try_on_runner(r, [](auto &prob, const RunControls &rc) { prob.initialize(rc); }); }
// one time step; trace rows as poro_host_run; work: see fill_work
int poro_host_runner_step(void *r, double *trace, int max_rows, int64_t *work) {
  try {
    return on_runner(r, [&](auto &prob, const RunControls &rc) { const int rows = prob.time_step(rc, trace, max_rows); if (work) fill_work(prob.work, work); return rows; });
  } catch (const std::exception &e) { g_err = e.what(); return -1; }
}
// action 0: snapshot the device state, 1: roll back to it
int poro_host_runner_state(void *r, int action) {
  return try_on_runner(r, [&](auto &prob, const RunControls &) { if (action) prob.restore_state(); else prob.save_state(); });
}
// roll back to the snapshot, then one time step, in ONE call (a benchmark that repeats a step pays one host-language round trip instead of two)
int poro_host_runner_restore_and_step(void *r, double *trace, int max_rows, int64_t *work) {
  return poro_host_runner_state(r, 1) != 0 ? -1 : poro_host_runner_step(r, trace, max_rows, work);
}
// tail of the time loop body (PoroelasticityFSS.h:409-411): shear strains, effective stresses and, with a directory, solution-NNNN.vtk
int poro_host_runner_postprocess(void *r, const char *output_dir, int corrected) {
  return try_on_runner(r, [&](auto &prob, RunControls rc) { rc.output_dir = output_dir ? output_dir : ""; rc.corrected_postprocessing = corrected != 0; prob.postprocess(rc); });
}
// the same with the Darcy velocity per cell appended to the file (CELL_DATA / VECTORS darcy_velocity) when darcy != 0
int poro_host_runner_postprocess_darcy(void *r, const char *output_dir, int corrected, int darcy) {
  return try_on_runner(r, [&](auto &prob, RunControls rc) { rc.output_dir = output_dir ? output_dir : ""; rc.corrected_postprocessing = corrected != 0;
    const bool was = prob.flow_controls.darcy_output; prob.flow_controls.darcy_output = darcy != 0;
    try { prob.postprocess(rc); } catch (...) { prob.flow_controls.darcy_output = was; throw; }
    prob.flow_controls.darcy_output = was; });
}
// the same with the switches of both post-processing families: darcy != 0 appends the Darcy velocity, stress != 0 behind it the cell stresses (CELL_DATA / TENSORS
// effective_stress, TENSORS total_stress, SCALARS mohr_coulomb, SCALARS von_mises; the criterion of poro_host_runner_mohr_coulomb, f = 0 without one)
int poro_host_runner_postprocess_fields(void *r, const char *output_dir, int corrected, int darcy, int stress) {
  return try_on_runner(r, [&](auto &prob, RunControls rc) { rc.output_dir = output_dir ? output_dir : ""; rc.corrected_postprocessing = corrected != 0;
    const bool was_d = prob.flow_controls.darcy_output, was_s = prob.stress_controls.stress_output;
    prob.flow_controls.darcy_output = darcy != 0; prob.stress_controls.stress_output = stress != 0;
    try { prob.postprocess(rc); } catch (...) { prob.flow_controls.darcy_output = was_d; prob.stress_controls.stress_output = was_s; throw; }
    prob.flow_controls.darcy_output = was_d; prob.stress_controls.stress_output = was_s; });
}
// Mechanical accounting (PoroElasticProblem::force_balance / force_history).  poro_host_runner_mohr_coulomb: the criterion of the runner's measures (on = 0: none).
// poro_host_runner_track_force: while on, every step appends its force balance to the history (initialize clears it).  poro_host_runner_force_history: record s of the
// history as 16 doubles in the order of poro_force_balance_terms (out may be NULL); returns the number of records, < 0 on error
int poro_host_runner_mohr_coulomb(void *r, int on, double cohesion, double friction_angle) {
  return try_on_runner(r, [&](auto &prob, const RunControls &) { prob.stress_controls.mohr_coulomb = on != 0; prob.stress_controls.cohesion = cohesion; prob.stress_controls.friction_angle = friction_angle; });
}
int poro_host_runner_track_force(void *r, int on) { return try_on_runner(r, [&](auto &prob, const RunControls &) { prob.stress_controls.force_balance = on != 0; }); }
int poro_host_runner_force_history(void *r, int s, double *out) {
  try {
    return on_runner(r, [&](auto &prob, const RunControls &) {
      const int n = (int)prob.force_history.size();
      if (out) {
        if (s < 0 || s >= n) throw std::runtime_error("runner_force_history: no such record");
        const poro_force_balance_terms &t = prob.force_history[s].terms;
        for (int k = 0; k < 3; ++k) { out[k] = t.reaction_sum[k]; out[3 + k] = t.free_row_sum[k]; out[6 + k] = t.traction_sum[k]; out[9 + k] = t.body_sum[k]; out[12 + k] = t.coupling_sum[k]; }
        out[15] = t.residual_l2;
      }
      return n;
    });
  } catch (const std::exception &e) { g_err = e.what(); return -1; }
}
// Flow accounting (PoroElasticProblem::flow_balance / flow_totals).  poro_host_runner_track_flow: flow_controls.flow_balance of the runner's problem - while on, every step adds dt * its
// terms to the totals.  poro_host_runner_flow_balance: the balance of the PRESENT state (nothing is accumulated by the call): terms[6] in the order of
// poro_flow_balance_terms; per prescribed label (at most max_labels) the label, the conservative outflow and the face-integrated discharge; totals[8] = steps accounted,
// the time integrals of storage_rate_strain, storage_rate_pressure, source_sum, outflow_prescribed, free_row_sum, the summed bounds dt sqrt(n) residual_l2, and the number
// of labels of the totals; total_outflow / total_discharge per label (same order).  Returns the number of labels, < 0 on error
int poro_host_runner_track_flow(void *r, int on) { return try_on_runner(r, [&](auto &prob, const RunControls &) { prob.flow_controls.flow_balance = on != 0; }); }
int poro_host_runner_flow_balance(void *r, double *terms, int32_t *labels, double *outflow, double *discharge, int max_labels, double *totals, double *total_outflow, double *total_discharge) {
  try {
    return on_runner(r, [&](auto &prob, const RunControls &rc) {
      const auto B = prob.flow_balance(rc);
      const poro_flow_balance_terms &t = B.terms;
      const double all[6] = {t.storage_rate_strain, t.storage_rate_pressure, t.source_sum, t.outflow_prescribed, t.free_row_sum, t.residual_l2};
      if (terms) std::copy(all, all + 6, terms);
      const int n = (int)B.labels.size();
      if (n > max_labels) throw std::runtime_error("runner_flow_balance: more prescribed labels than the caller has room for");
      for (int k = 0; k < n; ++k) { if (labels) labels[k] = B.labels[k]; if (outflow) outflow[k] = B.outflow_by_label[k]; if (discharge) discharge[k] = B.discharge_by_label[k]; }
      const auto &T = prob.flow_totals;
      if (totals) { const double tt[8] = {(double)T.steps, T.storage_strain, T.storage_pressure, T.source, T.outflow, T.free_rows, T.bound, (double)T.labels.size()}; std::copy(tt, tt + 8, totals); }
      for (size_t k = 0; k < T.labels.size() && (int)k < max_labels; ++k) { if (total_outflow) total_outflow[k] = T.outflow_by_label[k]; if (total_discharge) total_discharge[k] = T.discharge_by_label[k]; }
      return n;
    });
  } catch (const std::exception &e) { g_err = e.what(); return -1; }
}
// cumulative work counters since creation (same layout as poro_host_runner_step's `work`)
void poro_host_runner_work(void *r, int64_t *work) { on_runner(r, [&](auto &prob, const RunControls &) { fill_work(prob.work, work); }); }
// the preconditioners the driver chose for the current context (initialize, and again after every adapt): out[3] = displacement, pressure, projection (PORO_PREC_*)
void poro_host_runner_preconditioners(void *r, int32_t *out) {
  on_runner(r, [&](auto &p, const RunControls &) { out[0] = p.displacement_solver.control.preconditioner; out[1] = p.pressure_solver.control.preconditioner; out[2] = p.strain_projector.control.preconditioner; });
}
// the stopping rule of the pressure solve (PoroElasticPressureSolver.h:175: SolverControl(1000, 1e-8 * |R|)): ||g|| <= max(abs_tol, rel_tol ||R||).  Kept over initialize() and adapt()
int poro_host_runner_pressure_solver_tolerances(void *r, double abs_tol, double rel_tol) {
  if (!(abs_tol >= 0) || !(rel_tol >= 0)) { g_err = "pressure_solver_tolerances: tolerances must be >= 0"; return -1; }
  on_runner(r, [&](auto &p, const RunControls &) { p.pressure_solver.control.abs_tol = abs_tol; p.pressure_solver.control.rel_tol = rel_tol; });
  return 0;
}
void poro_host_runner_free(void *r) { delete static_cast<HostRunner *>(r); }

}  // extern "C"
