// extern "C" entry points of include/poroel_hip.h (the drop-in boundary); the host logic behind them lives in ctx_setup / ctx_comm / ctx_pcg / ctx_prec.hip, the entry points
// of the pressure and projection stages in ctx_pressure.hip, those of the per-cell coefficient fields in ctx_fields.hip.
#include <dlfcn.h>
#include <rccl/rccl.h>
#include <algorithm>
#include <array>
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

namespace {
// ---- pieces of poro_disp_assemble_system ------------------------------------------------------------------------------------------------
// lifting -(A_full g) on the free rows, from wh_u = A_full g (the unconstrained operator applied to the Dirichlet values)
void lifting_from_wh(poro_ctx *c) {
  la_fill(c->stream, c->lift_u.p, 0.0, c->n_u);
  la_axpy(c->stream, c->lift_u.p, -1.0, c->wh_u.p, c->n_u);
}

// throws unless max |a - b| <= rel_tol max |b|; a is overwritten with a - b
void throw_unless_close(poro_ctx *c, double *a, const double *b, int64_t n, double rel_tol, const char *what) {
  hipStream_t s = c->stream;
  la_axpy(s, a, -1.0, b, n);
  la_norm_partials(s, a, n, c->partials.p, c->partials.p + kMaxPartials);
  la_norm_partials(s, b, n, c->partials.p + 2 * kMaxPartials, c->partials.p + 3 * kMaxPartials);
  la_reduce_finish(s, c->partials.p, 4, c->red.p, 2 | 8);
  double h[4];
  PORO_HIP(hipMemcpyAsync(h, c->red.p, sizeof(h), hipMemcpyDeviceToHost, s));
  PORO_HIP(hipStreamSynchronize(s));
  if (!(h[1] <= rel_tol * h[3])) throw Error(std::string(what) + ": max diff " + std::to_string(h[1]) + " vs max " + std::to_string(h[3]));
}

// self-check of the structured CSR assembly (kernels_box.hip) against the coloured per-cell assembly
void check_box_assembly(poro_ctx *c, const AsmArgs &a) {
  hipStream_t s = c->stream;
  DevBuf<double> ref, lift_ref;
  ref.alloc(c->Au.nnz);
  ref.zero(s);
  lift_ref.alloc(c->n_u);
  lift_ref.zero(s);
  for_each_colour(c, [&](const int32_t *cells, int64_t n_cells) { asm_u_matrix(s, a, cells, n_cells, c->Au.rp.p, c->Au.col.p, ref.p, lift_ref.p); });
  throw_unless_close(c, ref.p, c->Au_val.p, c->Au.nnz, 1e-12, "structured CSR assembly disagrees with the per-cell assembly");
}

// self-check of the sum-factorised operator against the element-matrix gather on a synthetic vector (guards the FE-table / numbering
// assumptions of the structured path); both unconstrained
void check_sum_factorised_operator(poro_ctx *c) {
  hipStream_t s = c->stream;
  std::vector<double> hx(c->n_u);
  for (int64_t i = 0; i < c->n_u; ++i) hx[i] = std::sin(0.37 * (double)i);
  DevBuf<double> tx, t1, t2;
  tx.upload(hx);
  t1.alloc(c->n_u);
  t2.alloc(c->n_u);
  kron_apply(s, mf_args(c), tx.p, t1.p, false, c->n_cus);
  mf_apply(s, mf_args(c), tx.p, t2.p, false);
  throw_unless_close(c, t1.p, t2.p, c->n_u, 1e-11, "sum-factorised operator disagrees with the element-matrix operator");
}

// dictionary form of the Jacobi diagonal: on a uniform box only a few dozen distinct per-node triples exist, so the PCG kernels
// can read one class byte per node and a tiny table instead of 8 bytes per dof.  Built by de-duplicating the actual values of dinv_u;
// with more than 255 classes there is no dictionary
void build_diag_dictionary(poro_ctx *c) {
  std::vector<double> hd(c->n_u);
  PORO_HIP(hipMemcpyAsync(hd.data(), c->dinv_u.p, c->n_u * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  PORO_HIP(hipStreamSynchronize(c->stream));
  const int nc = c->dim;
  const int64_t nnode = c->n_u / nc;
  struct KeyHash {
    size_t operator()(const std::array<double, 3> &k) const {
      uint64_t h = 1469598103934665603ull;
      for (double v : k) {
        uint64_t b;
        std::memcpy(&b, &v, 8);
        h = (h ^ b) * 1099511628211ull;
        h ^= h >> 29;
      }
      return (size_t)h;
    }
  };
  std::unordered_map<std::array<double, 3>, int, KeyHash> dict;
  std::vector<uint8_t> cls(nnode);
  std::vector<double> tab;
  for (int64_t nd = 0; nd < nnode; ++nd) {
    std::array<double, 3> key{0, 0, 0};
    for (int k = 0; k < nc; ++k) key[k] = hd[nd * nc + k];
    auto it = dict.find(key);
    if (it == dict.end()) {
      if (dict.size() >= 255) return;
      it = dict.emplace(key, (int)dict.size()).first;
      for (int k = 0; k < nc; ++k) tab.push_back(key[k]);
    }
    cls[nd] = (uint8_t)it->second;
  }
  c->diag_u_cls.upload(cls);
  c->diag_u_tab.upload(tab);
}

// ---- displacement solves: one function per preconditioner family ---------------------------------------------------------------------------
// the operator of the displacement system, condensed on the fly where the mesh has constraint lists; apply(x, y, dot_partials) as apply_A_u
ApplyFn operator_u(poro_ctx *c) {
  return [c](const double *x, double *y, double *dp) {
    const int mode = c->operator_mode;
    if (!c->cons_u.n) return apply_A_u(c, x, y, mode, dp, false, dp ? c->scal.p : nullptr);
    // C^T A C: the search direction's hanging entries follow their masters, the product's hanging rows fold into the masters' rows
    la_cons_expand(c->stream, c->cons_u, const_cast<double *>(x), false);
    apply_A_u(c, x, y, mode, nullptr, false, nullptr, false);                 // the rank's partial product ...
    la_cons_reduce(c->stream, c->cons_u, y);                                   // ... folded ...
    exchange_add(c, y, c->n_u, c->comm.part.plane_u);                          // ... then summed over the interface
    return false;
  };
}

// constraints.distribute (:306) on the solution: the Dirichlet values and, with `expand`, the hanging entries from their masters
void finish_u(poro_ctx *c, bool expand) {
  la_set_constrained(c->stream, vec(c, PORO_VEC_U), c->dir_mask.p, c->dir_val.p, c->n_u);
  if (expand) la_cons_expand(c->stream, c->cons_u, vec(c, PORO_VEC_U), true);
}

// what every displacement solve shares.  `inert`: the rows kept out of the system (the Dirichlet rows, or those and the hanging ones); `dictionary`: the Jacobi diagonal in its
// class / table form where one was built
KrylovSystem krylov_u(poro_ctx *c, const uint8_t *inert, bool dictionary, int *hint) {
  KrylovSystem sys;
  sys.n = c->n_u; sys.plane = c->comm.part.plane_u;
  sys.x = vec(c, PORO_VEC_U); sys.b = vec(c, PORO_VEC_RHS_U);
  sys.apply = operator_u(c);
  sys.diag.full = c->dinv_u.p; sys.diag.ncomp = c->dim;
  if (dictionary && c->diag_u_cls.p) { sys.diag.cls = c->diag_u_cls.p; sys.diag.tab = c->diag_u_tab.p; }
  sys.inert = inert;
  sys.g = c->wg_u.p; sys.d = c->wd_u.p; sys.h = c->wh_u.p;
  sys.hint = hint;
  return sys;
}
// the vector an explicit displacement preconditioner writes
double *z_u(poro_ctx *c) {
  if (!c->wz_u.p) { c->wz_u.alloc(c->n_u); c->wz_u.zero(c->stream); }
  return c->wz_u.p;
}

// lambda_max(D^-1 A): on a uniform box all cells share one element matrix and lambda_max <= lambda_max(diag(K_e)^-1 K_e) holds rigorously
// (x^T A x = sum_e x_e^T K_e x_e <= mu sum_e x_e^T diag(K_e) x_e = mu x^T D x) but is loose (3.8 against 2.5 for Q2 hexahedra), so the working
// value is the Lanczos estimate (+5 %) capped by it.  Cached in c->cheb_lmax until the matrix is rebuilt
double chebyshev_lmax(poro_ctx *c, const KrylovSystem &sys) {
  if (c->cheb_lmax > 0) return c->cheb_lmax;
  const bool have_bound = box_fast_u(c) && c->Ke.p && !c->cons_u.n;      // (per-cell moduli: no single element matrix, the Lanczos estimate alone)
  if (have_bound) {
    std::vector<double> ke((size_t)c->dpc_u * c->dpc_u);
    PORO_HIP(hipMemcpyAsync(ke.data(), c->Ke.p, ke.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    PORO_HIP(hipStreamSynchronize(c->stream));
    const double bound = jacobi_scaled_lambda_max(c->dpc_u, ke);              // rigorous but loose
    c->cheb_lmax = std::min(bound, estimate_lmax_u(c, sys));
  } else {
    c->cheb_lmax = estimate_lmax_u(c, sys);
  }
  if (std::getenv("PORO_CHEB_VERBOSE")) std::fprintf(stderr, "[poro] lambda_max(D^-1 A_u) ~ %.6f\n", c->cheb_lmax);
  return c->cheb_lmax;
}

// default interval ratio: a few times lambda_min, which scales with h^2 (calibrated on box runs of 8^3 .. 72^3 cells).  Cached in c->cheb_ratio_default
double chebyshev_default_ratio(poro_ctx *c) {
  if (c->cheb_ratio_default > 0) return c->cheb_ratio_default;
  // from GLOBAL mesh sizes, so that every rank of a partitioned run builds the same polynomial (rank-local sizes gave uneven slabs different roots on
  // either side of a shared plane): the cell layers of the partitioned direction (slabs) / the cell count (general partitions) are summed over the ranks
  double h[2] = {(double)c->box.n[c->dim - 1], (double)c->n_cells};
  if (c->comm.multi()) {
    PORO_HIP(hipMemcpyAsync(c->red.p, h, sizeof(h), hipMemcpyHostToDevice, c->stream));
    allreduce_sum(c, c->red.p, 2);
    PORO_HIP(hipMemcpyAsync(h, c->red.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    PORO_HIP(hipStreamSynchronize(c->stream));
  }
  double nmax = 1;
  if (c->box.enabled) {
    for (int k = 0; k < c->dim; ++k) nmax = std::max(nmax, k == c->dim - 1 ? h[0] : (double)c->box.n[k]);
  } else {
    nmax = std::round(std::pow(h[1], 1.0 / c->dim));
  }
  c->cheb_ratio_default = std::min(400.0, std::max(10.0, (c->k_u == 2 ? 0.2 : 0.05) * nmax * nmax));
  return c->cheb_ratio_default;
}

// The polynomial of the Chebyshev preconditioner z = q(D^-1 A) D^-1 g: q of degree m for the interval [lmax / ratio, lmax].
// Only EVEN degrees are used: should an eigenvalue still exceed the assumed bound, it meets T_{m+1} outside [-1, 1], and q(lambda) lambda stays
// positive (the preconditioner SPD) exactly when m + 1 is odd.
// Root form: the residual polynomial of degree m + 1 is prod_i (1 - lambda / r_i) with the roots r_i of the Chebyshev polynomial shifted to
// [lmax / ratio, lmax]; z_1 = D^-1 g / r_0, z_{j+1} = z_j + D^-1 (g - A z_j) / r_j.  Same polynomial as the three-term recurrence
// (identical CG iteration counts in the prototype for every ordering at these degrees) with ONE extra stream per step (g) instead of two;
// the roots are taken alternately from both ends so that no run of small roots inflates the intermediate iterates
struct ChebPlan { int m; double lmax, ratio; std::vector<double> roots; };
ChebPlan chebyshev_plan(poro_ctx *c, const poro_solver_opts *opts, const KrylovSystem &sys) {
  ChebPlan p;
  p.m = opts->poly_degree > 0 ? opts->poly_degree : 6;
  if (p.m & 1) ++p.m;
  p.lmax = chebyshev_lmax(c, sys);
  // `omega` doubles as the interval ratio; anything below 4 (the SSOR relaxation 1.2 a caller may have left there, 0) means "default"
  p.ratio = opts->omega >= 4.0 ? opts->omega : chebyshev_default_ratio(c);
  const double lmin = p.lmax / p.ratio, theta = 0.5 * (p.lmax + lmin), delta = 0.5 * (p.lmax - lmin);
  const int m = p.m;
  std::vector<double> r(m + 1);
  for (int i = 0; i <= m; ++i) r[i] = theta - delta * std::cos(3.14159265358979323846 * (2 * i + 1) / (2.0 * (m + 1)));
  int lo = 0, hi = m;
  while (lo <= hi) {
    p.roots.push_back(r[hi--]);
    if (lo <= hi) p.roots.push_back(r[lo++]);
  }
  return p;
}

// m operator applications without dot products; on 3D boxes (one rank) the recurrence runs inside the structured operator kernel
int solve_u_chebyshev(poro_ctx *c, const poro_solver_opts *opts, poro_solve_info *info) {
  hipStream_t s = c->stream;
  KrylovSystem sys = krylov_u(c, c->cons_u.inert.p, true, c->pcg_hint_cheb_u);
  const ChebPlan plan = chebyshev_plan(c, opts, sys);
  const int m = plan.m;
  const std::vector<double> &roots = plan.roots;
  if (!c->cheb_z.p) {
    c->cheb_z.alloc(c->n_u);
    c->cheb_z.zero(s);
    c->cheb_t.alloc(c->n_u);
    c->cheb_t.zero(s);
  }
  const bool fusable = c->operator_mode == PORO_OP_MATRIX_FREE && c->mf_variant == 1 && box_fast_u(c) && kron_supported(c->dim, c->k_u) && c->diag_u_cls.p && !c->cons_u.n &&
                       !std::getenv("PORO_CHEB_UNFUSED");
  const bool fuse = fusable && !c->comm.multi();
  // slab partitions (3D): the fused kernel runs on every rank with its LOCAL partial product; on the two shared node planes it also leaves the raw partial, the neighbours
  // swap those planes and a plane-sized kernel redoes the update there with the complete sum (the same two numbers on both ranks: bitwise equal copies)
  const bool fuse_multi = fusable && c->comm.multi() && !c->comm.general && c->dim == 3;
  if (fuse_multi && c->cheb_side_lo.n < (size_t)c->comm.part.plane_u) {
    c->cheb_side_lo.alloc(c->comm.part.plane_u);
    c->cheb_side_hi.alloc(c->comm.part.plane_u);
  }
  const int64_t n_own = owned(c, c->n_u, c->comm.part.plane_u);

  // One step zn = zj + omega D^-1 (g - A zj) in its three forms.  dp != null (the last step of a call that asks for g . z) takes the block partials
  // of g . zn; each form returns whether it has left them there
  auto cheb_update = [&](const double *g, double *zn, double omega) {
    KronCheb kc;
    kc.g = g;
    kc.znew = zn;
    kc.omega = omega;
    kc.cls = c->diag_u_cls.p;
    kc.tab = c->diag_u_tab.p;
    return kc;
  };
  auto fused_kernel = [&](const double *zj, const KronCheb &kc, double *dp, const PcgScalars *pstate) {
    return sampled_dispatch(c, "apply_u_chebyshev_fused", [&](hipEvent_t e0, hipEvent_t e1) {
      return kron_apply(s, mf_args(c), zj, nullptr, true, c->n_cus, dp, e0, e1, pstate, &kc);
    });
  };
  auto step_fused_slabs = [&](const double *g, double *zj, double *zn, double omega, double *dp) {
    const poro_partition &pt = c->comm.part;
    const int64_t plane = pt.plane_u;
    KronCheb kc = cheb_update(g, zn, omega);
    kc.side_lo = pt.has_lower ? c->cheb_side_lo.p : nullptr;
    kc.side_hi = pt.has_upper ? c->cheb_side_hi.p : nullptr;
    (void)fused_kernel(zj, kc, nullptr, nullptr);
    if (pt.has_lower || pt.has_upper) {
      {
        Timed te(c, "halo_exchange");
        exchange_planes(c, c->cheb_side_lo.p, c->cheb_side_hi.p, plane);
      }
      la_cheb_fix_planes(s, zn, zj, g, kc.side_lo, c->comm.recv_lo.p, kc.side_hi, c->comm.recv_hi.p, sys.diag, omega, c->n_u, plane);
    }
    if (dp) la_dot_partials(s, g, zn, n_own, dp);
    return dp != nullptr;
  };
  auto step_fused = [&](const double *g, double *zj, double *zn, double omega, double *dp, const PcgScalars *pstate) {
    const KronCheb kc = cheb_update(g, zn, omega);
    if (dp) PORO_HIP(hipMemsetAsync(dp, 0, kMaxPartials * sizeof(double), s));
    const int slots = fused_kernel(zj, kc, dp, pstate);
    return dp && slots > 0;
  };
  auto step_unfused = [&](const double *g, double *zj, double *zn, double omega, double *dp) {
    sys.apply(zj, c->cheb_t.p, nullptr);
    la_cheb_step(s, zn, zj, g, c->cheb_t.p, sys.diag, omega, c->n_u, n_own, dp);
    return dp != nullptr;
  };
  sys.prec.z = z_u(c);
  sys.prec.gated = fuse;
  sys.prec.applications = m;
  sys.z1.out = (m % 2 == 0) ? sys.prec.z : c->cheb_z.p;     // z_1 = D^-1 g / r_0 rides with the residual update
  sys.z1.scale = 1.0 / roots[0];
  sys.prec.fn = [&](const double *g, double *z, const PrecCall &call) {
    Timed tm(c, "precondition_u_chebyshev");
    double *X[2] = {(m % 2 == 0) ? z : c->cheb_z.p, (m % 2 == 0) ? c->cheb_z.p : z};   // z_{j+1} lands in X[j & 1]; the last one (j = m) in z
    if (!call.z1_ready) la_cheb_first(s, X[0], g, sys.diag, 1.0 / roots[0], c->n_u);
    bool dot_done = false;
    for (int j = 1; j <= m; ++j) {
      const double omega = 1.0 / roots[j];
      double *zj = X[(j - 1) & 1], *zn = X[j & 1];
      double *dp = j == m ? call.gz_partials : nullptr;
      if (fuse_multi) dot_done = step_fused_slabs(g, zj, zn, omega, dp);
      else if (fuse) dot_done = step_fused(g, zj, zn, omega, dp, call.gate);
      else dot_done = step_unfused(g, zj, zn, omega, dp);
      ++c->cheb_applies;
    }
    return dot_done ? GzLeft::in_partials : GzLeft::nowhere;
  };
  const int rc = pcg(c, sys, opts, info);
  finish_u(c, true);
  return rc;   // (stream-ordered: pcg() returned after the finishing iteration, `distribute` follows in the stream)
}

// z = blockdiag(A_cc)^-1 g by fast diagonalisation: the same device-controlled SolverCG recurrence with an explicit preconditioner vector
int solve_u_fdm(poro_ctx *c, const poro_solver_opts *opts, poro_solve_info *info) {
  build_fdm_u(c);
  const FdmOct *oct = c->fdm_oct.built ? &c->fdm_oct : nullptr;
  const bool separate_gz = std::getenv("PORO_FDMO_SEPARATE_GZ") != nullptr;    // A/B hook, read once per solve: g . z by its own dot kernel, as before pass 2 produced it
  // Single-rank octant form: the iteration's live set is d + g + ONE octant-sized array that is h and z in turn, and x streams past the cache.
  //   h | z: the operator writes h and the residual update is its only reader; then transform pass 1 (fp32 mode: pass 3) rewrites the whole array as z, whose last reader is the
  //          direction update; then the operator writes h again.  The prologue has the same order (apply -> init_residual -> preconditioner -> first_direction).
  //   fp64 transforms run on z itself, without the scratch array (k_fdmo_pass: "in place"); the fp32 mode keeps its float scratch array.
  // PORO_FDMO_SEPARATE_BUFFERS (A/B hook, read once per solve): h in wh_u, the scratch array between the passes, plain accesses to x.  The timer family
  // "fdm_u_shared_buffers" counts the solves that ran on the shared layout (a count, no time; it counts whether or not the context's timing is on).
  const bool shared = oct && !oct->slab.on && !oct->planar && std::getenv("PORO_FDMO_SEPARATE_BUFFERS") == nullptr;
  if (shared) c->timers["fdm_u_shared_buffers"].enqueued++;
  if (oct && oct->per_dir) c->timers["fdm_u_per_direction_form"].enqueued++;      // (likewise a count: the solves that ran the per-direction form)
  const int precision = oct && oct->per_dir ? PORO_FDM_FP64 : c->fdm_precision;    // (the per-direction form has fp64 fragments only)
  double *const scratch = shared && precision != PORO_FDM_FP32 ? nullptr : c->fdm_oct.t.p;
  KrylovSystem sys = krylov_u(c, c->dir_mask.p, false, c->pcg_hint_fdm_u);
  if (shared) sys.h = c->fdm_oct.z.p;
  sys.oct.form = oct;
  sys.oct.stream_x = shared;
  sys.prec.z = c->wz_u.p;
  sys.prec.gated = oct != nullptr;     // every launch of an iteration is gated: overshooting is cheap
  sys.prec.decides_stop = oct && !oct->slab.on;   // octant and planar form: the first kernel of a call can run the stopping test (pcg decides whether it does)
  sys.prec.fn = [&](const double *g, double *z, const PrecCall &call) {
    // g, z in the layout of the form that is built (octants: three contiguous sweeps)
    if (!oct) {
      fdm_precondition_u(c, g, z);
      return GzLeft::nowhere;
    }
    // octant form: pass 2 leaves g . z in oct->gz_part; the first application of a solve is not asked for it (k_fdmo_first_direction's dot)
    const bool gz = call.gz_partials && !separate_gz;
    return fdm_precondition_u_form(c, g, z, call.gate, precision, scratch, gz ? c->fdm_oct.gz_part.p : nullptr, call.stop) ? GzLeft::in_octant_form : GzLeft::nowhere;
  };
  const int rc = pcg(c, sys, opts, info);
  finish_u(c, false);
  return rc;
}

// z = omega D^-1 g + P B_H^-1 P^T g: Jacobi on this mesh + the block fast diagonalisation of the underlying uniform box; SolverCG's recurrence with an
// explicit preconditioner vector
int solve_u_two_level(poro_ctx *c, const poro_solver_opts *opts, poro_solve_info *info) {
  if (!two_level_supported(c)) throw Error("PORO_PREC_TWO_LEVEL needs poro_desc.coarse (a refinement of a uniform box whose Dirichlet conditions cover whole faces)");
  const double om = opts->omega > 0 ? opts->omega : 1.0;
  KrylovSystem sys = krylov_u(c, c->cons_u.inert.p, false, c->pcg_hint_u);
  sys.prec.z = z_u(c);
  sys.prec.fn = [&](const double *g, double *z, const PrecCall &) {
    two_level_precondition_u(c, g, z, om);
    return GzLeft::nowhere;
  };
  const int rc = pcg(c, sys, opts, info);
  finish_u(c, true);
  return rc;
}

int solve_u_jacobi(poro_ctx *c, const poro_solver_opts *opts, poro_solve_info *info) {
  const int rc = pcg(c, krylov_u(c, c->cons_u.inert.p, true, c->pcg_hint_u), opts, info);
  finish_u(c, true);
  return rc;
}

}  // namespace

// The constant load vector of the displacement right-hand side and what is derived from it: neumann_u = the tractions, then (gravity on) + the body-force vector, always in
// this order from zero, so that the bits depend on the settings alone and not on the order of the calls; then the line flags of the box kernel.  Called where the
// matrix block is rebuilt and where gravity or the density changed (Gravity::loads_stale): the matrix, the diagonal, the lifting and the FDM tables stay
void poro::ctx_detail::assemble_loads_u(poro_ctx *c) {
  hipStream_t s = c->stream; const AsmArgs a = asm_args(c);
  c->neumann_u.zero(s);
  asm_u_neumann(s, a, c->bface_order.p, c->bface_group_off, c->bface_cell.p, c->bface_local.p, c->bface_id.p, c->n_neumann, c->neu_label.p, c->neu_comp.p, c->neu_val.p, c->neumann_u.p);
  if (c->grav.on) la_axpy(s, c->neumann_u.p, 1.0, c->grav.body_u.p, c->n_u);      // (never without gravity: no +0.0 enters the default)
  if (c->box_asm) {     // lift_u and neumann_u are final here: which of their lines the right-hand side kernel has to read
    if (c->rhs_u_flags.n != (size_t)box_rhs_u_flag_count(c->n_u)) c->rhs_u_flags.alloc((size_t)box_rhs_u_flag_count(c->n_u));
    box_rhs_u_flags(s, c->lift_u.p, c->neumann_u.p, c->n_u, c->rhs_u_flags.p);
  }
  c->grav.loads_stale = false;
}

// ======================================= extern "C" ================================================================
extern "C" {

const char *poro_last_error(void) { return g_err.c_str(); }
int poro_abi_version(void) { return PORO_ABI_VERSION; }

int poro_ctx_create(const poro_desc *desc, int device, int operator_mode, poro_ctx **out) {
  return guarded([&] {
    if (!desc || !out) throw Error("null argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) throw Error("no HIP device visible: this library has no CPU fallback");
    if (device < 0 || device >= ndev) throw Error("device index out of range");
    PORO_HIP(hipSetDevice(device));
    std::unique_ptr<poro_ctx> c(new poro_ctx());
    c->device = device; c->operator_mode = operator_mode;
    PORO_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    kron_prepare_device();   // function attributes are per device: opt in to the large dynamic LDS on THIS one
    kron_lm_prepare_device();
    { void *mbp = nullptr; PORO_HIP(hipHostMalloc(&mbp, sizeof(Mailbox), hipHostMallocDefault)); std::memset(mbp, 0, sizeof(Mailbox)); c->mailbox = static_cast<Mailbox *>(mbp); }
    setup(c.get(), desc);
    c->pres_host_loop = std::getenv("PORO_PRES_HOST_LOOP") != nullptr;      // A/B hook, read once per context: the pressure Newton loop call by call (poro_pres_newton_loop refuses)
    c->newton_gate.alloc(1); c->newton_gate.zero(c->stream); c->newton_rec.alloc(kNewtonRecord); c->newton_rec.zero(c->stream);
    if (desc->coarse.enabled) {
      // two-level preconditioner: the underlying uniform box becomes a context of its own on this context's stream
      if (!desc->coarse.box_problem || !desc->coarse.ptr || !desc->coarse.node || !desc->coarse.weight) throw Error("poro_desc.coarse: box_problem / ptr / node / weight missing");
      if (!desc->coarse.box_problem->box.enabled || desc->coarse.box_problem->coarse.enabled) throw Error("poro_desc.coarse.box_problem must be a uniform box (box.enabled) without a coarse space of its own");
      if (desc->coarse.box_problem->dim != desc->dim || desc->coarse.box_problem->degree_u != desc->degree_u) throw Error("poro_desc.coarse.box_problem: dimension / degree differ");
      if (!c->interleaved_u) throw Error("poro_desc.coarse needs node-interleaved displacement dofs");
      if (c->comm.part.n_ranks > 1 && !c->comm.general) throw Error("poro_desc.coarse on a slab partition: not supported (general partitions only, poro_partition.n_neighbours > 0)");
      // general partition: the interpolation rows are per local node, the restriction runs over the owned nodes [0, n_owned_u / dim)
      if (c->comm.general && (c->n_u % c->dim || c->comm.ifc_u.n_owned % c->dim))
        throw Error("poro_desc.coarse on a general partition needs whole displacement nodes: n_dofs_u and n_owned_u must be multiples of dim (node-interleaved numbering incl. ghost dofs)");
      poro_ctx *box = nullptr;
      if (poro_ctx_create(desc->coarse.box_problem, device, PORO_OP_MATRIX_FREE, &box) != 0) throw Error(std::string("poro_desc.coarse.box_problem: ") + poro_last_error());
      PORO_HIP(hipStreamSynchronize(box->stream)); (void)hipStreamDestroy(box->stream); box->stream = c->stream; box->borrowed_stream = true;
      box->fdm_form = PORO_FDM_FORM_DEFAULT; box->fdm_form_fixed = true;      // (the coarse solve keeps the default form of the block FDM, whatever PORO_FDMO_FORM says)
      box->comm.force_multi = false;      // the box is solved whole on every rank (replicated coarse solve): never the partitioned code path
      c->two_level.box = box;
      setup_two_level(c.get(), desc);
    }
    // diagnostic switch, read once here: the initial scatter mode of the general operator
    if (const char *v = std::getenv("PORO_MFG_SCATTER")) {
      const std::string m(v);
      if (m != "atomic" && m != "coloured") throw Error("PORO_MFG_SCATTER: atomic or coloured");
      if (m == "atomic" && !c->box.enabled) c->scatter_mode = PORO_SCATTER_ATOMIC;
    }
    // read once here as well: the initial transform precision of the displacement system's octant-form block FDM (so that unchanged drivers can run the fp32 mode)
    if (const char *v = std::getenv("PORO_FDMO_PRECISION")) {
      const std::string m(v);
      if (m != "fp32" && m != "fp64") throw Error("PORO_FDMO_PRECISION: fp32 or fp64");
      c->fdm_precision = m == "fp32" ? PORO_FDM_FP32 : PORO_FDM_FP64;
    }
    // and the initial form of that block FDM (poro_ctx_set_fdm_form); the nested coarse box above keeps the default whatever this says
    if (const char *v = std::getenv("PORO_FDMO_FORM")) {
      const std::string m(v);
      if (m != "per-direction" && m != "default") throw Error("PORO_FDMO_FORM: per-direction or default");
      c->fdm_form = m == "per-direction" ? PORO_FDM_FORM_PER_DIRECTION : PORO_FDM_FORM_DEFAULT;
    }
    // and the requested form of the displacement operator on boxes with layered moduli (poro_ctx_set_moduli_operator)
    if (const char *v = std::getenv("PORO_MODULI_OPERATOR")) {
      const std::string m(v);
      if (m != "structured" && m != "cells") throw Error("PORO_MODULI_OPERATOR: structured or cells");
      c->moduli_op = m == "structured" ? PORO_MODULI_OP_STRUCTURED : PORO_MODULI_OP_CELLS;
    }
    *out = c.release();
    return 0;
  });
}

// The structured form is honoured where moduli_structured_applies (common.hpp); elsewhere the request is recorded and the cell loop runs as before
int poro_ctx_set_moduli_operator(poro_ctx *c, int32_t form) {
  return guarded([&] {
    if (!c) throw Error("null argument");
    if (form != PORO_MODULI_OP_CELLS && form != PORO_MODULI_OP_STRUCTURED) throw Error("poro_ctx_set_moduli_operator: unknown form " + std::to_string(form) + " (PORO_MODULI_OP_CELLS or PORO_MODULI_OP_STRUCTURED)");
    PORO_HIP(hipSetDevice(c->device));
    const int before = c->moduli_op;
    c->moduli_op = form;
    try { sync_moduli_planes(c); } catch (...) { c->moduli_op = before; throw; }
    return 0;
  });
}
int poro_ctx_get_moduli_operator(poro_ctx *c, int32_t *requested, int32_t *effective) {
  return guarded([&] {
    if (!c || !requested || !effective) throw Error("null argument");
    *requested = c->moduli_op; *effective = moduli_structured(c) ? PORO_MODULI_OP_STRUCTURED : PORO_MODULI_OP_CELLS;
    return 0;
  });
}

int poro_ctx_set_scatter_mode(poro_ctx *c, int32_t mode) {
  return guarded([&] {
    if (!c) throw Error("null argument");
    if (mode != PORO_SCATTER_COLOURED && mode != PORO_SCATTER_ATOMIC) throw Error("poro_ctx_set_scatter_mode: unknown mode " + std::to_string(mode) + " (PORO_SCATTER_COLOURED or PORO_SCATTER_ATOMIC)");
    if (box_fast_u(c)) return 0;   // the structured kernels have no scatter: nothing to select (a box with per-cell moduli runs the general cell loop and takes the mode)
    PORO_HIP(hipSetDevice(c->device));
    if (mode == PORO_SCATTER_ATOMIC && c->operator_mode == PORO_OP_MATRIX_FREE) build_spatial_cells(c);   // (a CSR context that applies the matrix-free operator builds it then)
    c->scatter_mode = mode;
    return 0;
  });
}
int poro_ctx_get_scatter_mode(poro_ctx *c, int32_t *mode) {
  return guarded([&] { if (!c || !mode) throw Error("null argument"); *mode = c->scatter_mode; return 0; });
}

int poro_ctx_set_operator_form(poro_ctx *c, int32_t form) {
  return guarded([&] {
    if (!c) throw Error("null argument");
    if (form != PORO_OPFORM_GENERAL && form != PORO_OPFORM_HYBRID) throw Error("poro_ctx_set_operator_form: unknown form " + std::to_string(form) + " (PORO_OPFORM_GENERAL or PORO_OPFORM_HYBRID)");
    if (form == PORO_OPFORM_HYBRID && c->mod.kind) throw Error("poro_ctx_set_operator_form: PORO_OPFORM_HYBRID is not available while per-cell moduli are set - the box part of the hybrid operator is a constant-coefficient kernel");
    if (c->box.enabled) return 0;   // the structured kernels already run on every cell: nothing to select
    PORO_HIP(hipSetDevice(c->device));
    if (form == PORO_OPFORM_HYBRID) hybrid_enable(c);   // throws where the mesh cannot take it: the form stays as it was (GENERAL, or a HYBRID that was accepted before)
    c->operator_form = form;
    return 0;
  });
}
int poro_ctx_get_operator_form(poro_ctx *c, int32_t *form, int64_t *general_cells, int64_t *removed_box_cells) {
  return guarded([&] {
    if (!c || !form) throw Error("null argument");
    const bool hybrid = c->operator_form == PORO_OPFORM_HYBRID;
    *form = c->operator_form;
    if (general_cells) *general_cells = c->box.enabled ? 0 : hybrid ? c->hyb.n_fine_cells : c->n_cells;
    if (removed_box_cells) *removed_box_cells = hybrid ? c->hyb.n_removed : 0;
    return 0;
  });
}

// true where PORO_PREC_FDM of the displacement system runs in the single-rank 3D octant form.  Builds the block FDM where that is possible at all (one rank, 3D, separable
// Dirichlet faces) - the numerical symmetry check of the eigenvectors is part of the build, so only then is the answer final
static bool fdm_u_runs_octant(poro_ctx *c) {
  if (!c->fdm_u.built) {
    if (c->dim != 3 || c->comm.multi()) return false;
    analyse_fdm_u(c);
    if (c->fdm_u_state != 1) return false;
    build_fdm_u(c);
  }
  return c->fdm_oct.built && !c->fdm_oct.planar && !c->fdm_oct.slab.on && !c->fdm_oct.per_dir;
}
int poro_ctx_set_fdm_precision(poro_ctx *c, int32_t precision) {
  return guarded([&] {
    if (!c) throw Error("null argument");
    if (precision != PORO_FDM_FP64 && precision != PORO_FDM_FP32) throw Error("poro_ctx_set_fdm_precision: unknown precision " + std::to_string(precision) + " (PORO_FDM_FP64 or PORO_FDM_FP32)");
    c->fdm_precision = precision;   // (the fp32 fragments are uploaded with the fp64 ones when the block FDM is built: nothing to do here, and forms without fp32 kernels never look at it)
    return 0;
  });
}
int poro_ctx_get_fdm_precision(poro_ctx *c, int32_t *requested, int32_t *effective) {
  return guarded([&] {
    if (!c || !requested || !effective) throw Error("null argument");
    *requested = c->fdm_precision; *effective = PORO_FDM_FP64;
    if (c->fdm_precision == PORO_FDM_FP32) { PORO_HIP(hipSetDevice(c->device)); if (fdm_u_runs_octant(c)) *effective = PORO_FDM_FP32; }
    return 0;
  });
}

// The per-direction form is honoured by single-rank 3D contexts (never by the nested coarse box of a two-level preconditioner); elsewhere the request is recorded and ignored
static bool fdm_form_applies(const poro_ctx *c) { return c->dim == 3 && !c->comm.multi() && !c->fdm_form_fixed; }
int poro_ctx_set_fdm_form(poro_ctx *c, int32_t form) {
  return guarded([&] {
    if (!c) throw Error("null argument");
    if (form != PORO_FDM_FORM_DEFAULT && form != PORO_FDM_FORM_PER_DIRECTION) throw Error("poro_ctx_set_fdm_form: unknown form " + std::to_string(form) + " (PORO_FDM_FORM_DEFAULT or PORO_FDM_FORM_PER_DIRECTION)");
    if (form != c->fdm_form && c->fdm_u.built && fdm_form_applies(c)) { PORO_HIP(hipSetDevice(c->device)); release_fdm_u(c); }   // built in the other form: rebuilt at next use
    c->fdm_form = form;
    return 0;
  });
}
int poro_ctx_get_fdm_form(poro_ctx *c, int32_t *requested, int32_t *effective, int32_t split[3]) {
  return guarded([&] {
    if (!c || !requested || !effective) throw Error("null argument");
    *requested = c->fdm_form; *effective = PORO_FDM_RUNS_NODAL;
    int mask = 0;
    PORO_HIP(hipSetDevice(c->device));
    if (!c->fdm_u.built && !c->comm.multi()) { analyse_fdm_u(c); if (c->fdm_u_state == 1) build_fdm_u(c); }   // (a partitioned context builds collectively, at its first solve)
    const FdmOct &O = c->fdm_oct;
    if (c->fdm_u.built && O.built) {
      *effective = O.slab.on ? PORO_FDM_RUNS_SLAB : O.planar ? PORO_FDM_RUNS_PLANAR : O.per_dir ? PORO_FDM_RUNS_PER_DIRECTION : PORO_FDM_RUNS_OCTANT;
      mask = O.per_dir ? O.split_mask : O.planar ? (O.no == 4 ? 3 : 0) : 7;       // (slabs: the z butterfly sits next to the all-to-all)
    }
    if (split) for (int d = 0; d < 3; ++d) split[d] = (mask >> d) & 1;
    return 0;
  });
}

void poro_ctx_destroy(poro_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  timers_collect(c);
  for (hipEvent_t e : c->event_pool) (void)hipEventDestroy(e);
  c->event_pool.clear();
  if (c->comm.nccl_comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy((ncclComm_t)c->comm.nccl_comm);
  if (c->two_level.box) { poro_ctx_destroy(c->two_level.box); c->two_level.box = nullptr; }
  if (c->stream && !c->borrowed_stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

int poro_comm_unique_id(void *id128) {
  return guarded([&] { g_rccl.load(); ncclUniqueId id; PORO_NCCL(g_rccl.GetUniqueId(&id)); static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId"); std::memcpy(id128, &id, 128); return 0; });
}
int poro_ctx_comm_init_rccl(poro_ctx *c, const void *id128) {
  return guarded([&] {
    g_rccl.load(); PORO_HIP(hipSetDevice(c->device));
    ncclUniqueId id; std::memcpy(&id, id128, 128); ncclComm_t comm;
    PORO_NCCL(g_rccl.CommInitRank(&comm, c->comm.part.n_ranks, id, c->comm.part.rank));
    c->comm.nccl_comm = comm;
    // self-test of the data plane on the compute stream: an all-reduce of a known value and one grouped neighbour exchange
    // (to itself when there is a single rank), so a broken RCCL set-up fails here with a message instead of inside a solve
    const int nr = c->comm.part.n_ranks, rk = c->comm.part.rank;
    DevBuf<double> t; t.alloc(4);
    double h[4] = {1.0 + rk, 2.0, 100.0 + rk, -1.0};
    PORO_HIP(hipMemcpyAsync(t.p, h, sizeof(h), hipMemcpyHostToDevice, c->stream));
    PORO_NCCL(g_rccl.AllReduce(t.p, t.p, 2, ncclFloat64, ncclSum, comm, c->stream));
    const int up = (rk + 1) % nr, down = (rk + nr - 1) % nr;
    PORO_NCCL(g_rccl.GroupStart());
    PORO_NCCL(g_rccl.Send(t.p + 2, 1, ncclFloat64, up, comm, c->stream));
    PORO_NCCL(g_rccl.Recv(t.p + 3, 1, ncclFloat64, down, comm, c->stream));
    PORO_NCCL(g_rccl.GroupEnd());
    PORO_HIP(hipMemcpyAsync(h, t.p, sizeof(h), hipMemcpyDeviceToHost, c->stream)); PORO_HIP(hipStreamSynchronize(c->stream));
    if (h[0] != 0.5 * nr * (nr + 1) || h[1] != 2.0 * nr || h[3] != 100.0 + down) throw Error("RCCL self-test failed (all-reduce / send-recv returned wrong data)");
    // the two exchange patterns of the solver, on one double each: the bidirectional neighbour exchange of exchange_add and the
    // all-to-all of the partitioned fast diagonalisation
    {
      DevBuf<double> sb, rb; sb.alloc(nr + 2); rb.alloc(nr + 2);
      std::vector<double> hs(nr + 2), hr(nr + 2, -1.0);
      for (int q = 0; q < nr; ++q) hs[q] = 1000.0 * rk + q;
      hs[nr] = 7.0 + rk; hs[nr + 1] = 9.0 + rk;
      PORO_HIP(hipMemcpyAsync(sb.p, hs.data(), (nr + 2) * sizeof(double), hipMemcpyHostToDevice, c->stream));
      PORO_HIP(hipMemcpyAsync(rb.p, hr.data(), (nr + 2) * sizeof(double), hipMemcpyHostToDevice, c->stream));
      const bool has_up = rk + 1 < nr, has_dn = rk > 0;
      PORO_NCCL(g_rccl.GroupStart());
      if (has_up) { PORO_NCCL(g_rccl.Send(sb.p + nr, 1, ncclFloat64, rk + 1, comm, c->stream)); PORO_NCCL(g_rccl.Recv(rb.p + nr, 1, ncclFloat64, rk + 1, comm, c->stream)); }
      if (has_dn) { PORO_NCCL(g_rccl.Send(sb.p + nr + 1, 1, ncclFloat64, rk - 1, comm, c->stream)); PORO_NCCL(g_rccl.Recv(rb.p + nr + 1, 1, ncclFloat64, rk - 1, comm, c->stream)); }
      PORO_NCCL(g_rccl.GroupEnd());
      PORO_NCCL(g_rccl.GroupStart());
      for (int q = 0; q < nr; ++q) if (q != rk) { PORO_NCCL(g_rccl.Send(sb.p + q, 1, ncclFloat64, q, comm, c->stream)); PORO_NCCL(g_rccl.Recv(rb.p + q, 1, ncclFloat64, q, comm, c->stream)); }
      PORO_NCCL(g_rccl.GroupEnd());
      PORO_HIP(hipMemcpyAsync(hr.data(), rb.p, (nr + 2) * sizeof(double), hipMemcpyDeviceToHost, c->stream)); PORO_HIP(hipStreamSynchronize(c->stream));
      bool ok = true;
      if (has_up && hr[nr] != 9.0 + (rk + 1)) ok = false;          // the upper neighbour's "down" message
      if (has_dn && hr[nr + 1] != 7.0 + (rk - 1)) ok = false;      // the lower neighbour's "up" message
      for (int q = 0; q < nr; ++q) if (q != rk && hr[q] != 1000.0 * q + rk) ok = false;
      if (!ok) throw Error("RCCL self-test failed (neighbour exchange / all-to-all returned wrong data)");
    }
    return 0;
  });
}
int poro_ctx_comm_init_callbacks(poro_ctx *c, poro_allreduce_fn ar, poro_sendrecv_fn sr, void *user) { c->comm.ar = ar; c->comm.sr = sr; c->comm.user = user; return 0; }

int poro_ctx_synchronize(poro_ctx *c) { return guarded([&] { PORO_HIP(hipSetDevice(c->device)); PORO_HIP(hipStreamSynchronize(c->stream)); return 0; }); }

int poro_vec_set(poro_ctx *c, int which, const double *host, int64_t n) {
  return guarded([&] { PORO_HIP(hipSetDevice(c->device)); if (vec_len(c, which) != n) throw Error("vector length mismatch"); PORO_HIP(hipMemcpyAsync(vec(c, which), host, n * sizeof(double), hipMemcpyHostToDevice, c->stream)); PORO_HIP(hipStreamSynchronize(c->stream)); return 0; });
}
int poro_vec_get(poro_ctx *c, int which, double *host, int64_t n) {
  return guarded([&] {
    PORO_HIP(hipSetDevice(c->device)); if (vec_len(c, which) != n) throw Error("vector length mismatch");
    if (which == PORO_VEC_SOURCE_P) sync_source_vector(c);
    if (which == PORO_VEC_DIAG_U) la_copy(c->stream, vec(c, which), c->diag_u.p ? c->diag_u.p : c->diag_u_local.p, n);
    PORO_HIP(hipMemcpyAsync(host, vec(c, which), n * sizeof(double), hipMemcpyDeviceToHost, c->stream)); PORO_HIP(hipStreamSynchronize(c->stream)); return 0;
  });
}
int poro_vec_fill(poro_ctx *c, int which, double v) { return guarded([&] { PORO_HIP(hipSetDevice(c->device)); la_fill(c->stream, vec(c, which), v, vec_len(c, which)); return 0; }); }
int poro_vec_copy(poro_ctx *c, int dst, int src) {
  return guarded([&] { PORO_HIP(hipSetDevice(c->device)); if (vec_len(c, dst) != vec_len(c, src)) throw Error("vector length mismatch"); la_copy(c->stream, vec(c, dst), vec(c, src), vec_len(c, dst)); return 0; });
}
int poro_vec_axpy(poro_ctx *c, int y, double a, int x) {
  return guarded([&] { PORO_HIP(hipSetDevice(c->device)); if (vec_len(c, y) != vec_len(c, x)) throw Error("vector length mismatch"); la_axpy(c->stream, vec(c, y), a, vec(c, x), vec_len(c, y)); return 0; });
}
int poro_vec_norm(poro_ctx *c, int which, double *l2, double *linf) {
  return guarded([&] {
    PORO_HIP(hipSetDevice(c->device));
    const int64_t n = vec_len(c, which), plane = is_u_vec(which) ? c->comm.part.plane_u : c->comm.part.plane_p;
    la_norm_partials(c->stream, vec(c, which), owned(c, n, plane), c->partials.p, c->partials.p + kMaxPartials);
    post_sums_and_wait(c, c->partials.p, 2, 2, 1);   // linf stays rank-local under a partition (reporting only, PoroelasticityFSS.h:387-389)
    if (l2) *l2 = std::sqrt(c->mailbox->vals[0]); if (linf) *linf = c->mailbox->vals[1]; return 0;
  });
}

int poro_state_save(poro_ctx *c) {
  return guarded([&] {
    PORO_HIP(hipSetDevice(c->device));
    std::vector<double *> dst; std::vector<const double *> src; std::vector<int64_t> len;
    for (auto &kv : c->vec) { DevBuf<double> &d = c->vec_saved[kv.first]; if (d.n != kv.second.n) d.alloc(kv.second.n); dst.push_back(d.p); src.push_back(kv.second.p); len.push_back((int64_t)kv.second.n); }
    la_copy_many(c->stream, (int)dst.size(), dst.data(), src.data(), len.data());
    PORO_HIP(hipStreamSynchronize(c->stream)); return 0;
  });
}
int poro_state_restore(poro_ctx *c) {
  return guarded([&] {
    PORO_HIP(hipSetDevice(c->device));
    if (c->vec_saved.empty()) throw Error("state_restore without state_save");
    std::vector<double *> dst; std::vector<const double *> src; std::vector<int64_t> len;
    for (auto &kv : c->vec_saved) { dst.push_back(c->vec.at(kv.first).p); src.push_back(kv.second.p); len.push_back((int64_t)kv.second.n); }
    la_copy_many(c->stream, (int)dst.size(), dst.data(), src.data(), len.data());      // (one launch instead of two dozen)
    // the solves that follow repeat earlier ones: forget the iteration-count history, so that a measurement of a repeated step cannot profit from a perfect prediction
    for (int *h : {c->pcg_hint_u, c->pcg_hint_fdm_u, c->pcg_hint_cheb_u, c->pcg_hint_p, c->pcg_hint_proj}) h[0] = h[1] = 0;
    for (int &h : c->newton_hint) h = 0;
    return 0;
  });
}

int poro_disp_assemble_system(poro_ctx *c, int rebuild_matrix) {
  return guarded([&] {
    PORO_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream; const AsmArgs a = asm_args(c);
    if (rebuild_matrix || !c->matrix_built) {      // (poro_ctx_set_cell_moduli clears matrix_built: the next call rebuilds whatever the flag says)
      Timed tm(c, "assemble_u_matrix");
      c->lift_u.zero(s);                                                         // (neumann_u: assemble_loads_u below)
      if (c->operator_mode == PORO_OP_CSR && c->box_asm && !c->mod.kind) {
        // uniform box: one element matrix, every CSR entry written once by its owner (kernels_box.hip); the lifting -(A_full g) comes
        // from the unconstrained structured operator
        if (!c->Ke.p) c->Ke.alloc((size_t)c->dpc_u * c->dpc_u);
        asm_u_element_matrix(s, a, 0, c->Ke.p);
        box_asm_u_matrix(s, c->dim, c->k_u, c->box, c->Ke.p, c->Au, c->dir_mask.p, c->Au_val.p);
        if (!c->box_asm_checked && c->Au.nnz <= 60000000 && !std::getenv("PORO_DIAG_SKIP_SELFCHECK")) check_box_assembly(c, a);   // once
        c->box_asm_checked = true;
        mf_operator(c, c->dir_val.p, c->wh_u.p, false);
        lifting_from_wh(c);
        la_csr_diag(s, c->Au, c->Au_val.p, c->diag_u_local.p);
      } else if (c->operator_mode == PORO_OP_CSR) {
        c->Au_val.zero(s);
        for_each_colour(c, [&](const int32_t *cells, int64_t n_cells) { asm_u_matrix(s, a, cells, n_cells, c->Au.rp.p, c->Au.col.p, c->Au_val.p, c->lift_u.p); });
        la_csr_diag(s, c->Au, c->Au_val.p, c->diag_u_local.p);
      } else if (!box_fast_u(c)) {
        // general mesh (or a box with per-cell moduli), matrix-free: the diagonal and the lifting -(A_full g) come from the same quadrature-level cell loop
        // (coloured in either scatter mode: assembled data stay bitwise stable)
        count_mfg_launches(c, mfg_apply(s, a, c->color_cells.p, c->color_off, c->n_u, nullptr, c->diag_u_local.p, false, 1));
        count_mfg_launches(c, mfg_apply(s, a, c->color_cells.p, c->color_off, c->n_u, c->dir_val.p, c->wh_u.p, false, 0));
        lifting_from_wh(c);
      } else {
        asm_u_element_matrix(s, a, 0, c->Ke.p);
        mf_diag(s, mf_args(c), c->diag_u_local.p);
        // lifting: -(A_full g) on the free rows, through the unconstrained operator
        mf_operator(c, c->dir_val.p, c->wh_u.p, false);
        if (c->mf_variant == 1 && kron_supported(c->dim, c->k_u) && !std::getenv("PORO_DIAG_SKIP_SELFCHECK")) check_sum_factorised_operator(c);
        lifting_from_wh(c);
      }
      assemble_loads_u(c);
      if (!c->diag_u.p) c->diag_u.alloc(c->n_u);
      la_copy(s, c->diag_u.p, c->diag_u_local.p, c->n_u);
      exchange_add(c, c->diag_u.p, c->n_u, c->comm.part.plane_u);
      c->diag_u_cls.release(); c->diag_u_tab.release();
      if (!c->dinv_u.p) c->dinv_u.alloc(c->n_u);
      la_reciprocal(s, c->dinv_u.p, c->diag_u.p, c->n_u);
      la_mask_zero(s, c->dinv_u.p, c->cons_u.inert.p, c->n_u);                   // zero reciprocal = inert (Dirichlet or hanging) dof (DiagVec)
      if (c->operator_mode == PORO_OP_MATRIX_FREE && box_fast_u(c)) build_diag_dictionary(c);
      c->matrix_built = true; c->ilu_u_valid = false; c->cheb_lmax = 0;
    }
    if (c->grav.loads_stale) assemble_loads_u(c);      // gravity or the density changed since: the load vector alone, the matrix block stays
    {
      Timed tm(c, "assemble_u_rhs");
      double *rhs = vec(c, PORO_VEC_RHS_U);
      if (c->box_asm) box_rhs_u(s, c->dim, c->box_cpl, c->mat.biot_alpha, vec(c, PORO_VEC_P), c->lift_u.p, c->neumann_u.p, c->dir_mask.p, rhs, c->rhs_u_flags.p);
      else {
        la_fill(s, rhs, 0.0, c->n_u);                                            // rhs_vector = 0 (:204)
        for_each_colour(c, [&](const int32_t *cells, int64_t n_cells) { asm_u_rhs(s, a, cells, n_cells, vec(c, PORO_VEC_P), rhs); });
        la_rhs_u_finish(s, rhs, c->lift_u.p, c->neumann_u.p, c->dir_mask.p, c->n_u);
      }
    }
    if (c->cons_u.n) {
      // condensed right-hand side C^T (b - A x_inh), x_inh = the constraints' inhomogeneities (distribute_local_to_global, :280-286).  On a partition everything here is
      // the rank's PARTIAL vector: rows are folded into their masters first, the interface sums come last (a rank may hold a master without holding the constrained dof)
      double *rhs = vec(c, PORO_VEC_RHS_U);
      if (c->cons_u.any_inhom) {
        la_fill(s, c->wd_u.p, 0.0, c->n_u); la_cons_expand(s, c->cons_u, c->wd_u.p, true);
        if (c->operator_mode == PORO_OP_CSR) la_csr_spmv(s, c->Au, c->Au_val.p, c->wd_u.p, c->wh_u.p);
        else if (!box_fast_u(c)) {
          // general mesh: a set-up quantity like the lifting above, so coloured in either scatter mode (VEC_RHS_U stays bitwise stable); otherwise as mf_operator
          count_mfg_launches(c, mfg_apply(s, a, c->color_cells.p, c->color_off, c->n_u, c->wd_u.p, c->wh_u.p, true, 0));
          kron_fix_constrained(s, mf_args(c), c->wd_u.p, c->wh_u.p, nullptr, 0);
        } else mf_operator(c, c->wd_u.p, c->wh_u.p, true);
        la_mask_zero(s, c->wh_u.p, c->dir_mask.p, c->n_u);
        la_axpy(s, rhs, -1.0, c->wh_u.p, c->n_u);
      }
      la_cons_reduce(s, c->cons_u, rhs);
    }
    exchange_add(c, vec(c, PORO_VEC_RHS_U), c->n_u, c->comm.part.plane_u);
    // stream-ordered: the right-hand side is consumed by kernels of the same stream (a caller that wants the host to wait calls poro_ctx_synchronize)
    return 0;
  });
}

int poro_supports_preconditioner(poro_ctx *c, int32_t which_system, int32_t prec) { return c && !prec_refusal(c, which_system, prec); }
int poro_disp_solve(poro_ctx *c, const poro_solver_opts *opts, poro_solve_info *info) {
  return guarded([&] {
    PORO_HIP(hipSetDevice(c->device));
    if (!c->matrix_built) throw Error("disp_solve before disp_assemble_system");
    const int prec = opts->preconditioner;
    if (const char *why = prec_refusal(c, 0, prec, true)) throw Error(why);
    if (prec == PORO_PREC_ILU0 || prec == PORO_PREC_SSOR) {
      KrylovSystem sys = krylov_u(c, nullptr, false, nullptr);
      const int rc = pcg_csr_sweeps(c, c->Au, c->Au_val.p, c->ilu_u, c->ilu_u_valid, sys, opts, info);
      finish_u(c, false);
      PORO_HIP(hipStreamSynchronize(c->stream));
      return rc;
    }
    if (prec == PORO_PREC_CHEBYSHEV) return solve_u_chebyshev(c, opts, info);
    if (prec == PORO_PREC_FDM) return solve_u_fdm(c, opts, info);
    if (prec == PORO_PREC_TWO_LEVEL) return solve_u_two_level(c, opts, info);
    return solve_u_jacobi(c, opts, info);
  });
}

static void csr_of(poro_ctx *c, int which, CsrDev **A, double **val) {
  switch (which) {
    case PORO_MAT_A_U: if (c->operator_mode != PORO_OP_CSR) throw Error("A_u is matrix-free in this context"); *A = &c->Au; *val = c->Au_val.p; return;
    case PORO_MAT_MASS_P: *A = &c->Ap; *val = c->Mp.p; return;
    case PORO_MAT_LAPLACE_P: *A = &c->Ap; *val = c->Kp.p; return;
    case PORO_MAT_JACOBIAN_P: *A = &c->Ap; *val = c->Jp.p; return;
  }
  throw Error("unknown matrix id");
}
int poro_export_csr_size(poro_ctx *c, int which, int64_t *n_rows, int64_t *nnz) {
  return guarded([&] { CsrDev *A; double *v; csr_of(c, which, &A, &v); *n_rows = A->n; *nnz = A->nnz; return 0; });
}
int poro_export_csr(poro_ctx *c, int which, int64_t *row_ptr, int32_t *col, double *val) {
  return guarded([&] {
    PORO_HIP(hipSetDevice(c->device)); CsrDev *A; double *v; csr_of(c, which, &A, &v);
    PORO_HIP(hipStreamSynchronize(c->stream));
    PORO_HIP(hipMemcpy(row_ptr, A->rp.p, (A->n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost)); PORO_HIP(hipMemcpy(col, A->col.p, A->nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
    PORO_HIP(hipMemcpy(val, v, A->nnz * sizeof(double), hipMemcpyDeviceToHost)); return 0;
  });
}

int poro_apply_operator(poro_ctx *c, int which, const double *x_host, double *y_host) {
  return guarded([&] {
    PORO_HIP(hipSetDevice(c->device)); hipStream_t s = c->stream;
    const bool isu = which == PORO_MAT_A_U; const int64_t n = isu ? c->n_u : c->n_p;
    DevBuf<double> x, y; x.upload(x_host, n); y.alloc(n);
    if (isu) { if (!c->matrix_built) throw Error("apply A_u before disp_assemble_system"); apply_A_u(c, x.p, y.p, c->operator_mode); }
    else { CsrDev *A; double *v; csr_of(c, which, &A, &v); la_csr_spmv(s, *A, v, x.p, y.p); exchange_add(c, y.p, n, c->comm.part.plane_p); }
    PORO_HIP(hipMemcpyAsync(y_host, y.p, n * sizeof(double), hipMemcpyDeviceToHost, s)); PORO_HIP(hipStreamSynchronize(s)); return 0;
  });
}

int poro_apply_preconditioner_u(poro_ctx *c, int32_t preconditioner, const double *g_host, double *z_host, int32_t reps, double *seconds_per_apply) {
  return guarded([&] {
    PORO_HIP(hipSetDevice(c->device)); hipStream_t s = c->stream;
    if (!c->matrix_built) throw Error("apply_preconditioner_u before disp_assemble_system");
    DevBuf<double> g, z; g.upload(g_host, c->n_u); z.alloc(c->n_u); z.zero(s);
    if (preconditioner == PORO_PREC_FDM) {
      if (const char *why = prec_refusal(c, 0, preconditioner, true)) throw Error(why);
      build_fdm_u(c);
      FdmOct &O = c->fdm_oct;
      // octant form where the solver uses it: butterflies outside (H, H'), the three transform passes in between - the timed part, as inside PCG
      const int precision = O.built && O.per_dir ? PORO_FDM_FP64 : c->fdm_precision;      // (the per-direction form has fp64 fragments only)
      fdm_precondition_u_nodal(c, g.p, z.p, precision);
      auto once = [&]() { if (O.built) fdm_precondition_u_form(c, O.g.p, O.z.p, nullptr, precision, O.t.p); else fdm_precondition_u(c, g.p, z.p); };
      if (reps > 0 && seconds_per_apply) {
        EventPair ev(c); PORO_HIP(hipEventRecord(ev.e0, s));
        for (int k = 0; k < reps; ++k) once();
        PORO_HIP(hipEventRecord(ev.e1, s)); PORO_HIP(hipEventSynchronize(ev.e1));
        float ms = 0; PORO_HIP(hipEventElapsedTime(&ms, ev.e0, ev.e1)); *seconds_per_apply = ms * 1e-3 / reps;
      }
    } else if (preconditioner == PORO_PREC_JACOBI) {
      PORO_HIP(hipMemcpyAsync(z.p, g.p, c->n_u * sizeof(double), hipMemcpyDeviceToDevice, s));
      la_pointwise_mul(s, z.p, c->dinv_u.p, c->n_u);
    } else throw Error("apply_preconditioner_u: PORO_PREC_JACOBI or PORO_PREC_FDM");
    PORO_HIP(hipMemcpyAsync(z_host, z.p, c->n_u * sizeof(double), hipMemcpyDeviceToHost, s)); PORO_HIP(hipStreamSynchronize(s)); return 0;
  });
}

int poro_bench_operator(poro_ctx *c, int which, int operator_mode, int reps, double *seconds_per_apply) {
  return guarded([&] {
    PORO_HIP(hipSetDevice(c->device)); hipStream_t s = c->stream;
    if (which != PORO_MAT_A_U) throw Error("bench_operator: only A_u");
    if (!c->matrix_built) throw Error("bench_operator before disp_assemble_system");
    if (operator_mode != c->operator_mode) throw Error("bench_operator: context was created with the other operator mode");
    std::vector<double> hx(c->n_u); for (int64_t i = 0; i < c->n_u; ++i) hx[i] = std::sin(0.37 * (double)i);   // SURVEY 8d synthetic vector
    DevBuf<double> x, y; x.upload(hx); y.alloc(c->n_u);
    for (int k = 0; k < 3; ++k) apply_A_u(c, x.p, y.p, operator_mode);
    EventPair ev(c); const hipEvent_t e0 = ev.e0, e1 = ev.e1;
    PORO_HIP(hipEventRecord(e0, s));
    for (int k = 0; k < reps; ++k) apply_A_u(c, x.p, y.p, operator_mode);
    PORO_HIP(hipEventRecord(e1, s)); PORO_HIP(hipEventSynchronize(e1));
    float ms = 0; PORO_HIP(hipEventElapsedTime(&ms, e0, e1));
    *seconds_per_apply = ms * 1e-3 / reps; return 0;
  });
}

int poro_timers_reset(poro_ctx *c) { return guarded([&] { PORO_HIP(hipSetDevice(c->device)); timers_collect(c); c->timers.clear(); c->timing = true; c->timing_stride = 1; return 0; }); }
int poro_timers_enable(poro_ctx *c, int on) { return guarded([&] { PORO_HIP(hipSetDevice(c->device)); timers_collect(c); c->timing = on != 0; c->timing_stride = on > 1 ? on : 1; return 0; }); }
int poro_timers_get(poro_ctx *c, const char *name, double *seconds, int64_t *launches) {
  return guarded([&] {
    PORO_HIP(hipSetDevice(c->device)); timers_collect(c);
    auto it = c->timers.find(name);
    // sampled families: the measured time is scaled to all launches of the family (mean sampled duration x launches enqueued)
    const bool have = it != c->timers.end() && it->second.launches > 0;
    if (seconds) *seconds = have ? it->second.seconds * (double)std::max(it->second.enqueued, it->second.launches) / (double)it->second.launches : 0.0;
    if (launches) *launches = it == c->timers.end() ? 0 : std::max(it->second.enqueued, it->second.launches);
    return 0;
  });
}

}  // extern "C"
