// The per-cell coefficient fields of a context: k / mu of the pressure system (poro_ctx_set / get_cell_permeability) or its diagonal tensor diag(kx, ky[, kz]) / mu
// (poro_ctx_set / get_cell_permeability_tensor) - one field, c->perm, of 1 or dim components - and Lame lambda, shear G of the displacement system
// (poro_ctx_set / get_cell_moduli) - and gravity with its per-cell bulk density (poro_ctx_set / get_gravity, poro_ctx_set / get_cell_density), which changes right-hand
// sides only.  What they share - the refusals, the caller's cell order -> lattice order, the classification by layers, the host state - is
// cell_field.hpp; each setter adds its value checks, its device state and what it invalidates.  A setter that throws leaves the context as it was: the device state
// changes first, then the host state, then the caches go
#include <cmath>
#include <cstring>
#include "common.hpp"
#include "ctx_internal.hpp"
#include "moduli_planes.hpp"

using namespace poro;
using namespace poro::ctx_detail;

namespace {
// the refusals every entry point words alike; `who` is its name, `name` its name for the count
void refuse_partitioned(const poro_ctx *c, const std::string &who) { if (c->comm.part.n_ranks > 1 || c->comm.multi()) throw Error(who + ": partitioned contexts are not supported (one rank only)"); }
void check_count(const poro_ctx *c, const std::string &who, const char *name, int64_t n) { if (n != c->n_cells) throw Error(who + ": " + name + " is " + std::to_string(n) + ", the context has " + std::to_string(c->n_cells) + " cells"); }
std::vector<int32_t> download_cell_dofs_p(poro_ctx *c) {
  std::vector<int32_t> dofs((size_t)c->n_cells * c->nv);
  PORO_HIP(hipMemcpyAsync(dofs.data(), c->cell_dofs_p.p, dofs.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  PORO_HIP(hipStreamSynchronize(c->stream));
  return dofs;
}
// F takes the arrays; on boxes and tensor-product grids (c->lines) it classifies them on the lattice - dofs: cell_dofs_p - and the lattice-ordered copies come back
// used: the components that are taken (CellField::set)
template <int N> std::array<std::vector<double>, N> take(const poro_ctx *c, CellField<N> &F, const double *const (&comp)[N], const std::vector<int32_t> &dofs, const char *who, int used = N) {
  if (!c->lines.on) return F.set(comp, c->n_cells, nullptr, 0, nullptr, used);
  const std::vector<int64_t> order = cell_lattice_order(c->dim, c->lines.n, dofs.data(), c->nv, c->n_cells, who);      // (lines.n is 1 beyond dim)
  return F.set(comp, c->n_cells, &order, c->dim, c->lines.n, used);
}
// the getters: *kind always; the arrays that are asked for (out[a] != null) while a field is set
template <class Field, int N> int give(poro_ctx *c, Field poro_ctx::*field, double *const (&out)[N], int64_t n, int32_t *kind, const std::string &who, const char *name) {
  return guarded([&] {
    if (!c || !kind) throw Error("null argument");
    const CellField<N> &F = c->*field;
    *kind = F.kind;
    for (int a = 0; a < N && F.kind; ++a) if (out[a]) { check_count(c, who, name, n); std::memcpy(out[a], F.host[a].data(), (size_t)n * sizeof(double)); }
    return 0;
  });
}

// Kp = K_kappa over the coloured cell loop, w = [n_cells][ncomp] weights (w == null: the plain Laplace matrix, bit for bit what setup() assembled: same kernel, same order)
void assemble_laplace_p(poro_ctx *c, const double *w, int ncomp = 1) {
  hipStream_t s = c->stream; const AsmArgs a = asm_args(c);
  c->Kp.zero(s);
  for_each_colour(c, [&](const int32_t *cells, int64_t n_cells) { asm_p_matrices(s, a, cells, n_cells, c->Ap.rp.p, c->Ap.col.p, nullptr, c->Kp.p, nullptr, w, ncomp); });
}
// what goes with every change of the pressure system's field, the caches of line pivots among it
void invalidate_pressure(poro_ctx *c) {
  c->jac_dt = -1; c->ilu_J_valid = false;
  for (auto &L : c->perm.line) { L.built = false; L.a = -1; }
}
// ---- gravity: the two vectors from the present settings (kernels_gravity.hip).  Uniform boxes take the closed-form node kernels, every other mesh the coloured cell loop
int64_t box_nodes(const poro_ctx *c, int k) { return (int64_t)(k * c->box.n[0] + 1) * (k * c->box.n[1] + 1) * (c->dim == 3 ? k * c->box.n[2] + 1 : 1); }
// body_u = sum_c rho_c int_c g . phi_i; the load vector that carries it is rebuilt by the next poro_disp_assemble_system (assemble_loads_u), and only that
void build_gravity_body(poro_ctx *c) {
  poro_ctx::Gravity &G = c->grav; hipStream_t s = c->stream;
  G.loads_stale = true;
  if (!G.on) { if (G.body_u.p) { PORO_HIP(hipStreamSynchronize(s)); G.body_u.release(); } return; }
  if (G.body_u.n != (size_t)c->n_u) G.body_u.alloc(c->n_u);
  const double *lattice = G.dens.kind ? G.dens.lattice.p : nullptr;
  Timed tm(c, "gravity_body_u");
  if (c->box.enabled && (c->k_u == 1 || c->k_u == 2) && box_nodes(c, c->k_u) * c->dim == c->n_u && (!G.dens.kind || lattice)) box_body_u(s, c->dim, c->k_u, c->box, lattice, G.rho_b, G.g, G.body_u.p);
  else {
    const AsmArgs a = asm_args(c);
    G.body_u.zero(s);
    for_each_colour(c, [&](const int32_t *cells, int64_t n_cells) { asm_u_body(s, a, cells, n_cells, G.dens.kind ? G.dens.cell.p : nullptr, G.rho_b, G.g, G.body_u.p); });
  }
}
// flux_p = -sum_c rho_f int_c (kappa_c g) . grad(phi_i) with the permeability the context holds, and src_p = src_local + flux_p, what the pressure residual reads
void build_gravity_flux(poro_ctx *c) {
  poro_ctx::Gravity &G = c->grav; const poro_ctx::Perm &P = c->perm; hipStream_t s = c->stream;
  if (!G.flux_on()) { if (G.flux_p.p) { PORO_HIP(hipStreamSynchronize(s)); G.flux_p.release(); G.src_p.release(); } return; }
  if (G.flux_p.n != (size_t)c->n_p) { G.flux_p.alloc(c->n_p); G.src_p.alloc(c->n_p); }
  const int ncomp = P.kind ? P.ncomp : 1;
  {
    Timed tm(c, "gravity_flux_p");
    if (c->box.enabled && box_nodes(c, 1) == c->n_p && (!P.kind || P.lattice.p)) box_gravity_p(s, c->dim, c->box, P.kind ? P.lattice.p : nullptr, ncomp, c->mat.k_over_mu, G.rho_f, G.g, G.flux_p.p);
    else {
      const AsmArgs a = asm_args(c);
      G.flux_p.zero(s);
      for_each_colour(c, [&](const int32_t *cells, int64_t n_cells) { asm_p_gravity(s, a, cells, n_cells, P.kind ? P.cell.p : nullptr, ncomp, c->mat.k_over_mu, G.rho_f, G.g, G.flux_p.p); });
    }
  }
  la_copy(s, G.src_p.p, c->src_local.p, c->n_p);
  la_axpy(s, G.src_p.p, 1.0, G.flux_p.p, c->n_p);
}

// NULL to either setter: back to poro_material.k_over_mu, the plain Laplace matrix bit for bit
int back_to_constant(poro_ctx *c) {
  poro_ctx::Perm &P = c->perm;
  if (!P.kind) return 0;
  assemble_laplace_p(c, nullptr);
  P.clear(); P.ncomp = 0; P.cell.release(); P.lattice.release();
  invalidate_pressure(c);
  build_gravity_flux(c);
  return 0;
}
// The two setters: k_over_mu is [n_cells][ncomp], ncomp = 1 (one k / mu per cell) or dim (diag(kx, ky[, kz]) / mu, x first); `who` names the entry point in the refusals
int set_permeability(poro_ctx *c, const double *k_over_mu, int64_t n_cells, int ncomp, const std::string &who) {
  return guarded([&] {
    if (!c) throw Error("null argument");
    PORO_HIP(hipSetDevice(c->device));
    if (!k_over_mu) return back_to_constant(c);
    refuse_partitioned(c, who);
    check_count(c, who, "n_cells", n_cells);
    std::vector<double> comp[3];
    for (int d = 0; d < ncomp; ++d) comp[d].resize((size_t)n_cells);
    for (int64_t i = 0; i < n_cells; ++i)
      for (int d = 0; d < ncomp; ++d) {
        const double v = comp[d][(size_t)i] = k_over_mu[i * ncomp + d];
        if (!(std::isfinite(v) && v > 0)) throw Error(who + ": " + (ncomp > 1 ? "component " + std::to_string(d) + " of cell " : "value of cell ") + std::to_string(i) + " is not finite and > 0");
      }
    CellField<3> F;
    const auto lattice = take(c, F, {comp[0].data(), comp[1].data(), comp[2].data()}, c->lines.on ? download_cell_dofs_p(c) : std::vector<int32_t>(), who.c_str(), ncomp);
    poro_ctx::Perm &P = c->perm;
    P.cell.upload(k_over_mu, (size_t)n_cells * ncomp);
    if (c->box.enabled && c->lines.on) {
      std::vector<double> planes; planes.reserve((size_t)n_cells * ncomp);
      for (int d = 0; d < ncomp; ++d) planes.insert(planes.end(), lattice[d].begin(), lattice[d].end());
      P.lattice.upload(planes);
    } else P.lattice.release();
    assemble_laplace_p(c, P.cell.p, ncomp);
    static_cast<CellField<3> &>(P) = std::move(F); P.ncomp = ncomp;
    invalidate_pressure(c);
    build_gravity_flux(c);      // (while gravity is on: the Darcy gravity flux follows the field)
    return 0;
  });
}
}  // namespace

// the plane table of the structured operator for layered moduli goes with the field, the request and what the context is: called wherever one of them changes
void poro::ctx_detail::sync_moduli_planes(poro_ctx *c) {
  poro_ctx::Moduli &M = c->mod;
  if (c->moduli_op != PORO_MODULI_OP_STRUCTURED || !moduli_structured_applies(c)) { if (M.planes.p) { PORO_HIP(hipStreamSynchronize(c->stream)); M.planes.release(); } return; }
  if ((int)M.layer[0].size() != c->box.n[2] || M.layer[1].size() != M.layer[0].size()) throw Error("structured moduli operator: the field's layers do not match the box");
  const std::vector<double> t = moduli_plane_table(c->k_u, M.layer[0], M.layer[1]);
  PORO_HIP(hipStreamSynchronize(c->stream));      // (an operator application that reads the old table may still be in flight)
  M.planes.upload(t);
}

extern "C" {

int poro_ctx_set_cell_permeability(poro_ctx *c, const double *k_over_mu, int64_t n_cells) { return set_permeability(c, k_over_mu, n_cells, 1, "poro_ctx_set_cell_permeability"); }
int poro_ctx_get_cell_permeability(poro_ctx *c, double *out, int64_t n_cells, int32_t *kind) {
  if (c && kind && c->perm.ncomp > 1)      // a tensor is set: its kind; the values belong to the other getter
    return guarded([&] {
      *kind = c->perm.kind;
      if (out) throw Error("poro_ctx_get_cell_permeability: a permeability tensor is set, its values come from poro_ctx_get_cell_permeability_tensor");
      return 0;
    });
  return give(c, &poro_ctx::perm, {out, (double *)nullptr, (double *)nullptr}, n_cells, kind, "poro_ctx_get_cell_permeability", "n_cells");
}

// Per-cell diagonal tensor diag(kx, ky[, kz]) / mu, k_over_mu[cell][component], x first
int poro_ctx_set_cell_permeability_tensor(poro_ctx *c, const double *k_over_mu, int64_t n_cells) { return set_permeability(c, k_over_mu, n_cells, c ? c->dim : 0, "poro_ctx_set_cell_permeability_tensor"); }
int poro_ctx_get_cell_permeability_tensor(poro_ctx *c, double *out, int64_t n_cells, int32_t *kind) {
  if (c && kind && c->perm.ncomp == 1) { *kind = 0; return 0; }      // one k / mu per cell is set: no tensor
  if (!c || !out || !c->perm.kind) return give(c, &poro_ctx::perm, {(double *)nullptr, (double *)nullptr, (double *)nullptr}, n_cells, kind, "poro_ctx_get_cell_permeability_tensor", "n_cells");
  std::vector<double> comp[3]; const int dim = c->dim;
  for (int d = 0; d < dim; ++d) comp[d].resize((size_t)std::max<int64_t>(n_cells, c->n_cells));
  const int rc = give(c, &poro_ctx::perm, {comp[0].data(), comp[1].data(), dim == 3 ? comp[2].data() : (double *)nullptr}, n_cells, kind, "poro_ctx_get_cell_permeability_tensor", "n_cells");
  if (rc == 0) for (int64_t i = 0; i < n_cells; ++i) for (int d = 0; d < dim; ++d) out[i * dim + d] = comp[d][(size_t)i];
  return rc;
}

// Per-cell Lame lambda and shear modulus G.  Everything the displacement system derives from the moduli is dropped here and rebuilt by the next
// poro_disp_assemble_system: the assembled matrix, the Jacobi diagonal and its dictionary, the lifting, Ke, lambda_max of the Chebyshev form, the ILU factor, the FDM tables
int poro_ctx_set_cell_moduli(poro_ctx *c, const double *lame_lambda, const double *shear_G, int64_t n_cells) {
  return guarded([&] {
    if (!c) throw Error("null argument");
    PORO_HIP(hipSetDevice(c->device));
    poro_ctx::Moduli &M = c->mod;
    auto invalidate = [&] {
      c->matrix_built = false; c->ilu_u_valid = false; c->cheb_lmax = 0;
      c->diag_u_cls.release(); c->diag_u_tab.release();
      release_fdm_u(c);
      for (int *h : {c->pcg_hint_u, c->pcg_hint_fdm_u, c->pcg_hint_cheb_u}) h[0] = h[1] = 0;
    };
    if (!lame_lambda && !shear_G) {
      if (!M.kind) return 0;
      PORO_HIP(hipStreamSynchronize(c->stream));
      M.clear(); M.cell.release(); M.node.release(); M.planes.release();
      invalidate();
      return 0;
    }
    if (!lame_lambda || !shear_G) throw Error("poro_ctx_set_cell_moduli: lame_lambda and shear_G come together (one of the two arrays is NULL)");
    refuse_partitioned(c, "poro_ctx_set_cell_moduli");
    if (c->operator_form == PORO_OPFORM_HYBRID) throw Error("poro_ctx_set_cell_moduli: the context runs PORO_OPFORM_HYBRID, whose box part is a constant-coefficient kernel (select PORO_OPFORM_GENERAL first)");
    check_count(c, "poro_ctx_set_cell_moduli", "n_cells", n_cells);
    for (int64_t i = 0; i < n_cells; ++i) {
      const double l = lame_lambda[i], g = shear_G[i];
      if (!(std::isfinite(l) && std::isfinite(g))) throw Error("poro_ctx_set_cell_moduli: moduli of cell " + std::to_string(i) + " are not finite");
      if (!(g > 0)) throw Error("poro_ctx_set_cell_moduli: shear_G of cell " + std::to_string(i) + " is not > 0");
      if (!(3 * l + 2 * g > 0)) throw Error("poro_ctx_set_cell_moduli: 3 lambda + 2 G of cell " + std::to_string(i) + " is not > 0");
    }
    const std::vector<int32_t> dofs = download_cell_dofs_p(c);
    CellField<2> F;
    take(c, F, {lame_lambda, shear_G}, dofs, "poro_ctx_set_cell_moduli");      // (a layered array's values are its layer means)
    // nodal constants of the pressure space: the arithmetic mean over the cells that touch the dof
    const std::vector<double> &lam = F.host[0], &G = F.host[1];
    std::vector<double> node((size_t)2 * c->n_p, 0.0), pair((size_t)2 * n_cells); std::vector<int32_t> touch((size_t)c->n_p, 0);
    for (int64_t e = 0; e < n_cells; ++e) {
      pair[2 * e] = lam[e]; pair[2 * e + 1] = G[e];
      for (int v = 0; v < c->nv; ++v) { const int32_t d = dofs[(size_t)e * c->nv + v]; node[2 * (size_t)d] += lam[e]; node[2 * (size_t)d + 1] += G[e]; touch[d]++; }
    }
    for (int64_t i = 0; i < c->n_p; ++i) {
      if (!touch[i]) { node[2 * i] = c->mat.lame_lambda; node[2 * i + 1] = c->mat.shear_G; continue; }      // (a dof no cell of this context touches)
      node[2 * i] /= touch[i]; node[2 * i + 1] /= touch[i];
    }
    PORO_HIP(hipStreamSynchronize(c->stream));
    M.cell.upload(pair); M.node.upload(node);
    static_cast<CellField<2> &>(M) = std::move(F);
    invalidate();
    sync_moduli_planes(c);
    return 0;
  });
}
int poro_ctx_get_cell_moduli(poro_ctx *c, double *lambda_out, double *G_out, int64_t n, int32_t *kind) { return give(c, &poro_ctx::mod, {lambda_out, G_out}, n, kind, "poro_ctx_get_cell_moduli", "n"); }

// Gravity.  Right-hand sides only: the body-force vector rides in the load vector behind the tractions, the Darcy gravity flux beside the well source; nothing the operators,
// the preconditioners or the Krylov drivers read changes, and nothing is invalidated but the load vector (rebuilt by the next poro_disp_assemble_system)
int poro_ctx_set_gravity(poro_ctx *c, const double *g, double bulk_density, double fluid_density) {
  return guarded([&] {
    if (!c) throw Error("null argument");
    PORO_HIP(hipSetDevice(c->device));
    poro_ctx::Gravity &G = c->grav;
    double gv[3] = {0, 0, 0}; bool on = false;
    for (int d = 0; g && d < c->dim; ++d) {
      if (!std::isfinite(g[d])) throw Error("poro_ctx_set_gravity: component " + std::to_string(d) + " of g is not finite");
      gv[d] = g[d]; on = on || g[d] != 0.0;
    }
    if (!(std::isfinite(bulk_density) && bulk_density >= 0)) throw Error("poro_ctx_set_gravity: bulk_density is not finite and >= 0");
    if (!(std::isfinite(fluid_density) && fluid_density >= 0)) throw Error("poro_ctx_set_gravity: fluid_density is not finite and >= 0");
    for (int d = 0; d < 3; ++d) G.g[d] = on ? gv[d] : 0.0;
    G.on = on; G.rho_b = bulk_density; G.rho_f = fluid_density;
    build_gravity_body(c); build_gravity_flux(c);
    return 0;
  });
}
int poro_ctx_get_gravity(poro_ctx *c, double *g, double *bulk_density, double *fluid_density, int32_t *on) {
  return guarded([&] {
    if (!c) throw Error("null argument");
    for (int d = 0; g && d < c->dim; ++d) g[d] = c->grav.g[d];
    if (bulk_density) *bulk_density = c->grav.rho_b;
    if (fluid_density) *fluid_density = c->grav.rho_f;
    if (on) *on = c->grav.on ? 1 : 0;
    return 0;
  });
}
// Per-cell bulk density in place of the scalar of poro_ctx_set_gravity (kept while gravity is off, used when it comes on)
int poro_ctx_set_cell_density(poro_ctx *c, const double *rho, int64_t n_cells) {
  return guarded([&] {
    if (!c) throw Error("null argument");
    PORO_HIP(hipSetDevice(c->device));
    poro_ctx::Gravity::Density &D = c->grav.dens;
    if (!rho) {
      if (!D.kind) return 0;
      PORO_HIP(hipStreamSynchronize(c->stream));
      D.clear(); D.cell.release(); D.lattice.release();
      if (c->grav.on) build_gravity_body(c);
      return 0;
    }
    refuse_partitioned(c, "poro_ctx_set_cell_density");
    check_count(c, "poro_ctx_set_cell_density", "n_cells", n_cells);
    for (int64_t i = 0; i < n_cells; ++i)
      if (!(std::isfinite(rho[i]) && rho[i] > 0)) throw Error("poro_ctx_set_cell_density: value of cell " + std::to_string(i) + " is not finite and > 0");
    CellField<1> F;
    const auto lattice = take(c, F, {rho}, c->lines.on ? download_cell_dofs_p(c) : std::vector<int32_t>(), "poro_ctx_set_cell_density");
    PORO_HIP(hipStreamSynchronize(c->stream));
    D.cell.upload(rho, (size_t)n_cells);
    if (c->box.enabled && c->lines.on) D.lattice.upload(lattice[0]); else D.lattice.release();
    static_cast<CellField<1> &>(D) = std::move(F);
    if (c->grav.on) build_gravity_body(c);
    return 0;
  });
}
int poro_ctx_get_cell_density(poro_ctx *c, double *out, int64_t n_cells, int32_t *kind) {
  if (!c || !kind) return guarded([&]() -> int { throw Error("null argument"); });
  return guarded([&] {
    const CellField<1> &F = c->grav.dens;
    *kind = F.kind;
    if (out && F.kind) { check_count(c, "poro_ctx_get_cell_density", "n_cells", n_cells); std::memcpy(out, F.host[0].data(), (size_t)n_cells * sizeof(double)); }
    return 0;
  });
}
// The two gravity vectors alone (no tractions, no well source; rank-partial sums on a partition); zeros while gravity is off or fluid_density is 0
int poro_get_gravity_vectors(poro_ctx *c, double *body_u, double *flux_p) {
  return guarded([&] {
    if (!c) throw Error("null argument");
    PORO_HIP(hipSetDevice(c->device));
    const poro_ctx::Gravity &G = c->grav;
    if (body_u) { if (G.on) PORO_HIP(hipMemcpyAsync(body_u, G.body_u.p, (size_t)c->n_u * sizeof(double), hipMemcpyDeviceToHost, c->stream)); else std::memset(body_u, 0, (size_t)c->n_u * sizeof(double)); }
    if (flux_p) { if (G.flux_on()) PORO_HIP(hipMemcpyAsync(flux_p, G.flux_p.p, (size_t)c->n_p * sizeof(double), hipMemcpyDeviceToHost, c->stream)); else std::memset(flux_p, 0, (size_t)c->n_p * sizeof(double)); }
    PORO_HIP(hipStreamSynchronize(c->stream));
    return 0;
  });
}

}  // extern "C"
