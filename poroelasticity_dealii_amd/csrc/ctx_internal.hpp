// Declarations shared by the host-logic translation units of the HIP back end (ctx*.hip); not part of the C-ABI.
#pragma once
#include <rccl/rccl.h>
#include <functional>
#include <string>
#include <vector>
#include "common.hpp"
#include "whole_faces.hpp"
#include "fdm_tables.hpp"

namespace poro {
namespace ctx_detail {

extern thread_local std::string g_err;
inline int ipow(int b, int e) { int r = 1; while (e--) r *= b; return r; }
// the body of an extern "C" entry point: what it throws becomes poro_last_error() and the return value -1
template <class F> int guarded(F &&f) {
  try { return f(); }
  catch (const std::exception &e) { g_err = e.what(); return -1; }
}
// fn(cells, n_cells) once per colour of the cell colouring (one launch each: the cells of a colour share no dof)
template <class F> void for_each_colour(poro_ctx *c, F &&fn) {
  for (size_t k = 0; k + 1 < c->color_off.size(); ++k)
    fn(c->color_cells.p + c->color_off[k], c->color_off[k + 1] - c->color_off[k]);
}

// ---- RCCL, resolved at run time so single-GPU use has no dependency on it (ctx_comm.hip) ----------------------------------------
struct Rccl {
  void *lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  const char *(*GetErrorString)(ncclResult_t) = nullptr;
  void load();
};
extern Rccl g_rccl;
#define PORO_NCCL(x) do { ncclResult_t r_ = (x); if (r_ != ncclSuccess) throw poro::Error(std::string(#x) + " -> " + poro::ctx_detail::g_rccl.GetErrorString(r_)); } while (0)

// ---- timing: HIP events on the launch stream around kernel families, drawn from a per-context pool (ctx_comm.hip) ---------------
hipEvent_t event_get(poro_ctx *c);
struct Timed {
  poro_ctx *c; Timer *t = nullptr; hipEvent_t a = nullptr, b = nullptr;
  Timed(poro_ctx *c_, const char *name);
  ~Timed();
};
void timers_collect(poro_ctx *c);
// A dispatch that carries its own start / stop events (the kernel's own duration, without the gaps to its neighbours in the stream).
// begin_sampled_dispatch counts one dispatch of `family` (only while timing is on) and returns its timer when this one is to carry events,
// with the stream already drained for it; null otherwise.  sampled_dispatch calls launch(e0, e1) with such events or with (nullptr, nullptr).
Timer *begin_sampled_dispatch(poro_ctx *c, const char *family);
template <class Launch> auto sampled_dispatch(poro_ctx *c, const char *family, Launch &&launch) {
  Timer *t = begin_sampled_dispatch(c, family);
  if (!t) return launch(nullptr, nullptr);
  hipEvent_t e0 = event_get(c), e1 = event_get(c);
  auto r = launch(e0, e1);
  t->pending.emplace_back(e0, e1);
  t->launches++;
  return r;
}
// a start / stop event pair that is returned to the context's pool on every exit path
struct EventPair {
  poro_ctx *c; hipEvent_t e0, e1;
  explicit EventPair(poro_ctx *c_) : c(c_), e0(event_get(c_)), e1(event_get(c_)) {}
  ~EventPair() { c->event_pool.push_back(e0); c->event_pool.push_back(e1); }
  EventPair(const EventPair &) = delete; EventPair &operator=(const EventPair &) = delete;
};
// device -> host scalars through the pinned mailbox (no copy engine, no stream synchronisation)
void post_and_wait(poro_ctx *c, const double *dev_src, int n, const PcgScalars *sc = nullptr);
void post_sums_and_wait(poro_ctx *c, const double *partials, int n_sets, int max_mask, int n_allreduce);
void newton_post_and_wait(poro_ctx *c, const double *partials_inf);      // one rank: c->newton_rec + max |p| -> mailbox->vals[0 .. kNewtonRecord)
void count_strip_launches(poro_ctx *c, int n);      // ctx_prec.hip

// ---- communication (ctx_comm.hip) ---------------------------------------------------------------------------------------------------
void setup_general_partition(poro_ctx *c, const poro_desc *d);
void exchange_planes(poro_ctx *c, const double *send_lo, const double *send_hi, int64_t plane);
void exchange_add(poro_ctx *c, double *v, int64_t n, int64_t plane);
void allreduce_sum(poro_ctx *c, double *dev, int n);                                          // a few scalars (at most kScalarSlots)
void allreduce_sum_vec(poro_ctx *c, double *dev, int64_t n, const char *timer);              // a vector of any length, timed under `timer`
int64_t owned(poro_ctx *c, int64_t n, int64_t plane);
AsmArgs asm_args(poro_ctx *c);
MfArgs mf_args(poro_ctx *c);
void mf_operator(poro_ctx *c, const double *x, double *y, bool constrained);
void mfg_operator(poro_ctx *c, const double *x, double *y, bool constrained);   // general cell loop, mode 0, in the context's scatter mode
void build_spatial_cells(poro_ctx *c);
void assemble_loads_u(poro_ctx *c);     // (ctx.hip) neumann_u = tractions (+ the body-force vector while gravity is on) and the box kernel's line flags of it
void sync_moduli_planes(poro_ctx *c);   // (ctx_fields.hip) uploads the plane table of the structured operator for layered moduli where that form is requested and applies, drops it elsewhere
// ---- hybrid operator form (ctx_hybrid.hip) ---------------------------------------------------------------------------------------------------
void hybrid_enable(poro_ctx *c);                                               // derives the plan at the first call (host work, uploads, a stream synchronise) and checks it; throws where the mesh cannot take the form
void hybrid_operator(poro_ctx *c, const double *x, double *y, bool constrained);   // one application in the context's scatter mode (the Dirichlet rows are left to the caller, as by mfg_operator)
void count_mfg_launches(poro_ctx *c, int n);                                   // timer family "mfg_cell_kernels": cell-loop kernel launches of mfg_apply (a count, no time)
double *vec(poro_ctx *c, int which);
int64_t vec_len(poro_ctx *c, int which);
bool is_u_vec(int which);
// the device vector `which` where it belongs to the displacement (or the pressure) space; throws otherwise, in the name of the entry point
inline const double *space_vector(poro_ctx *c, int which, bool displacement, const char *name) {
  auto it = c->vec.find(which);
  if (it == c->vec.end()) throw Error("unknown vector id " + std::to_string(which));
  const bool ok = displacement ? is_u_vec(which) && (int64_t)it->second.n == c->n_u : !is_u_vec(which) && (int64_t)it->second.n == c->n_p;
  if (!ok) throw Error(std::string(name) + ": vector " + std::to_string(which) + (displacement ? " is not a displacement-space vector" : " is not a pressure-space vector"));
  return it->second.p;
}
// the post-processing entry points (ctx_flux.hip, ctx_stress.hip) run on one rank
inline void require_single_rank(poro_ctx *c, const char *name) {
  if (!c) throw Error("null argument");
  if (c->comm.part.n_ranks > 1) throw Error(std::string(name) + ": not implemented on partitioned contexts (n_ranks > 1)");
}
bool apply_A_u(poro_ctx *c, const double *x, double *y, int mode, double *dot_partials = nullptr, bool fix_rows = true, const PcgScalars *pcg_state = nullptr,
               bool exchange = true /* false: leave the rank's partial product (the caller folds constrained rows first) */);

// ---- Krylov drivers (ctx_pcg.hip) -----------------------------------------------------------------------------------------------------
// The operator: y = A x, consistent on the shared planes of a partition.  dh_partials != null (inside pcg()'s iteration only): the launch may be gated on c->scal, and a kernel that
// can leaves the block partials of x . y there; returns whether it did (false: the driver runs its own dot kernel).
typedef std::function<bool(const double *x, double *y, double *dh_partials)> ApplyFn;
// An explicit preconditioner: z = P^-1 g as a sequence of launches on the stream.  PrecCall is what the driver asks of ONE call:
struct PrecCall {
  const PcgScalars *gate = nullptr;   // the device-side "solve finished" flag the launches may test.  Null wherever it does not describe this solve: before pcg_scalars_start
                                      // (the first call of a solve; c->scal still holds the previous solve's state), in the single-reduction driver, and for a preconditioner that is not `gated`
  double *gz_partials = nullptr;      // where to leave the block partials of g . z over the owned rows; null: do not produce g . z (the driver's next kernel does)
  bool z1_ready = false;              // the residual update has already stored KrylovSystem::z1.scale D^-1 g in z1.out
  PcgStopTest stop;                   // gg_part != null (only where prec.decides_stop): the call's first kernel runs the iteration's stopping test and the whole call is skipped when it holds
};
enum class GzLeft { nowhere, in_partials /* PrecCall::gz_partials */, in_octant_form /* FdmOct::gz_part, which k_fdmo_update_d reads */ };   // where a call left g . z; nowhere: the driver runs a dot kernel
typedef std::function<GzLeft(const double *g, double *z, const PrecCall &)> PrecFn;

// One linear system A x = b as the three drivers see it; filled once per solve (ctx.hip: krylov_u, ctx_pressure.hip: solve_q1 fill what is common to a space)
struct KrylovSystem {
  int64_t n = 0, plane = 0;            // local length; dofs of one shared plane (slab partitions)
  double *x = nullptr; const double *b = nullptr;
  ApplyFn apply;
  DiagVec diag;                        // reciprocal Jacobi diagonal (read by PORO_PREC_JACOBI and for z1)
  const uint8_t *inert = nullptr;      // rows kept out of the system (nullable)
  double *g = nullptr, *d = nullptr, *h = nullptr;   // work vectors: residual, direction, A d
  int cg1_set = 0;                     // which of poro_ctx::cg1_w / cg1_z the single-reduction driver uses (0: displacement-sized, 1: pressure-sized)
  int *hint = nullptr;                 // iteration counts of the last two solves of this system (read for the batch sizes, then updated); nullable
  struct { PrecFn fn;                  // empty: Jacobi / none by poro_solver_opts::preconditioner
           double *z = nullptr;        // the vector the driver hands to fn (octant layout: Octant::form->z instead)
           bool gated = false;         // every launch of fn tests PrecCall::gate: iterations enqueued behind the finishing one cost ~1 us per launch
           bool decides_stop = false;  // (gated, one rank) fn hands PrecCall::stop to its first kernel: the finishing iteration skips the preconditioner
           int applications = 0;       // operator applications inside one call (a polynomial's degree): counted in poro_solve_info::operator_applications
  } prec;
  struct { const FdmOct *form = nullptr;   // non-null (pcg() only, needs prec.fn): residual and z live in this octant (one rank) / quadrant (slabs) layout, `g` is unused
           bool stream_x = false;      // h shares form->z's allocation: x streams past the cache in the direction update
  } oct;
  struct { double *out = nullptr; double scale = 0; } z1;   // out != null: the residual update also stores scale D^-1 g_new there (a polynomial preconditioner's first iterate)
};
int pcg(poro_ctx *c, const KrylovSystem &sys, const poro_solver_opts *opts, poro_solve_info *info);
double dot_host(poro_ctx *c, const double *a, const double *b, int64_t n);
// SSOR / ILU(0) by opts->preconditioner on the CSR matrix (A, val): fills sys.apply and sys.prec, runs the host-driven form.  lu, lu_valid: the ILU(0) factor and whether it belongs to val
int pcg_csr_sweeps(poro_ctx *c, CsrDev &A, const double *val, DevBuf<double> &lu, bool &lu_valid, KrylovSystem &sys, const poro_solver_opts *opts, poro_solve_info *info);
double estimate_lmax_u(poro_ctx *c, const KrylovSystem &sys);   // of the displacement system: its operator, Jacobi diagonal and inert rows

// ---- fast-diagonalisation preconditioners (ctx_prec.hip) ------------------------------------------------------------------------------
bool fdm_p_supported(poro_ctx *c);
bool fdm_pj_supported(poro_ctx *c);      // prescribed pressures on whole faces of a box / tensor grid, one rank
// the two table sets of the Q1 systems (poro_ctx::q1_free, q1_fixed): every end free | the ends of the prescribed faces removed (never built without prescribed pressures)
enum class Q1Set { free_ends, fixed_ends };
inline FdmQ1 &q1_set(poro_ctx *c, Q1Set which) { return which == Q1Set::fixed_ends ? c->q1_fixed : c->q1_free; }
void build_fdm_q1(poro_ctx *c, Q1Set which);
int slab_layout(poro_ctx *c, SlabLayout &L, int nodes_per_cell, int64_t ncol_total);
const char *prec_refusal(poro_ctx *c, int which_system, int prec, bool solving = false);   // null: usable; else why not (valid until the thread's next call)
void alltoall_blocks(poro_ctx *c, double *send, double *recv, int64_t blk, bool self_in_place = false /* the caller has already put its own block into recv */);
void setup_two_level(poro_ctx *c, const poro_desc *d);                // uploads P and its transpose (poro_desc.coarse)
bool two_level_supported(poro_ctx *c);
bool two_level_supported_p(poro_ctx *c);
bool two_level_supported_pj(poro_ctx *c);  // ... for the pressure Jacobian with prescribed rows: the coarse box carries them as whole faces (its second table set is the coarse solve)
void two_level_precondition_p(poro_ctx *c, double a, double kappa, const double *dinv, const double *g, double *z, double omega, const uint8_t *inert, Q1Set coarse_set = Q1Set::free_ends);   // z = omega D^-1 g + P (a M_H + kappa K_H)^-1 P^T g, 0 on the inert rows; Q1Set::fixed_ends: the coarse matrix without its prescribed rows
void two_level_precondition_u(poro_ctx *c, const double *g, double *z, double omega);   // z = omega D^-1 g + P B_H^-1 P^T g
bool fdm_precondition_u_form(poro_ctx *c, const double *g_form, double *z_form, const PcgScalars *gate, int precision, double *scratch, double *gz_part = nullptr, const PcgStopTest &stop = PcgStopTest{});   // c->fdm_oct is built: g, z in its layout (slab / planar / octant form); precision, scratch, gz_part: of the octant form's passes
void fdm_precondition_u_nodal(poro_ctx *c, const double *g, double *z, int precision);   // nodal g -> the form that is built (or the nodal kernels of fdm_precondition_u) -> nodal z
void fdm_precondition_p(poro_ctx *c, double a, const double k[3], const double *g, double *z, Q1Set which = Q1Set::free_ends);
void fdm_precondition_p_layered(poro_ctx *c, double a, const double *g, double *z, Q1Set which = Q1Set::free_ends);   // a per-cell coefficient is set: the line-solve form with c->perm.layer (exact for kind 1)
void analyse_fdm_u(poro_ctx *c);
void build_fdm_u(poro_ctx *c);
FdmuLineArgs fdmu_line_args(poro_ctx *c);   // per-cell moduli, after build_fdm_u: the arguments of the line-solve kernels (kernels_fdmu_line.hip)
void release_fdm_u(poro_ctx *c);   // frees what build_fdm_u made; the next use builds again (a change of the requested form)
void fdm_precondition_u(poro_ctx *c, const double *g, double *z);

// ---- pressure and projection systems (ctx_pressure.hip) ------------------------------------------------------------------------------------
// The numbers of the pressure equation at one time step: the residual's storage term is c_strain (ev - ev0) + c_pres (p - p_old), its flux term kappa K p (a per-cell k / mu:
// kappa = 1 and the field sits in Kp / the stencil), src the right-hand side vector (the well, + the Darcy gravity flux while that is on); strain_update: d eps_v = strain_update dp
struct PressureCoeffs { double c_strain, c_pres, kappa, strain_update; const double *src; };
PressureCoeffs pressure_coeffs(poro_ctx *c, double dt);
// rows = the uncondensed, rank-partial residual rows of PORO_VEC_P / P_OLD / EPSV / EPSV0 in the context's form (constant stencil, per-cell stencil or CSR); tmp: scratch of n_p.
// No timer scope of its own.  gate: the constant stencil alone, throws on the other two
void pressure_residual_rows(poro_ctx *c, const PressureCoeffs &k, double *tmp, double *rows, const PcgScalars *gate = nullptr);

// ---- mesh adaptation (ctx_adapt.hip) ------------------------------------------------------------------------------------------------------
// rows a caller hands in (interpolation / transfer): ptr[0] == 0, ptr ascending over n_rows rows, every column in [0, n_cols); throws before anything is uploaded
void validate_rows(const int64_t *ptr, const int32_t *col, const double *weight, int64_t n_rows, int64_t n_cols, const std::string &what);
void build_kelly_tables(poro_ctx *c);

// ---- set-up (ctx_setup.hip) -------------------------------------------------------------------------------------------------------------
void setup(poro_ctx *c, const poro_desc *d);
void sync_source_vector(poro_ctx *c);

}  // namespace ctx_detail
}  // namespace poro
