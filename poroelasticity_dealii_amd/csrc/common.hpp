// Shared declarations of the HIP back end (gfx950 only): device buffers, the context behind the
// opaque poro_ctx handle and the launch wrappers of every kernel family.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <map>
#include <memory>
#include <type_traits>
#include <stdexcept>
#include <string>
#include <list>
#include <vector>
#include "../../include/poroel_hip.h"
#include "fdm_tables.hpp"      // poro::Error (declared there: that header compiles without this one) and LineTables, the 1D tables of a grid line
#include "cell_field.hpp"      // poro::CellField, the host state of a per-cell coefficient field
#include "newton_record.hpp"   // the record of the pressure Newton loop's batches (host-only)

namespace poro {

#define PORO_HIP(x)                                                                                   \
  do { hipError_t e_ = (x); if (e_ != hipSuccess) throw poro::Error(std::string(#x) + " -> " + hipGetErrorString(e_)); } while (0)

template <class T> struct DevBuf {
  T *p = nullptr; size_t n = 0;
  DevBuf() = default; DevBuf(const DevBuf &) = delete; DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { release(); }
  void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
  void alloc(size_t n_) { release(); n = n_; if (n) PORO_HIP(hipMalloc((void **)&p, n * sizeof(T))); }
  void zero(hipStream_t s) { if (n) PORO_HIP(hipMemsetAsync(p, 0, n * sizeof(T), s)); }
  void upload(const T *h, size_t n_) { alloc(n_); if (n) PORO_HIP(hipMemcpy(p, h, n * sizeof(T), hipMemcpyHostToDevice)); }
  void upload(const std::vector<T> &h) { upload(h.data(), h.size()); }
};

constexpr int kMaxPartials = 1024;   // grid cap of every reducing kernel = number of per-block partial sums
constexpr int kScalarSlots = 32;

// device-resident scalars of a PCG solve (no host round trip inside the iteration)
struct PcgScalars {
  double dh, gg, gz;         // reductions of the current iteration (after all-reduce)
  double gh2[2];             // g.z of the previous iteration (ping-pong by iteration parity)
  double alpha, beta;
  double tol, res0, res;
  int32_t it, done, converged, max_iter, finishing;
  int32_t stop;              // the iteration's stopping decision where it is made in front of the preconditioner call (PcgStopTest): 0 go on, 1 converged, 2 max_iter reached
};
// The stopping test of iteration `it`, handed to the FIRST kernel of a gated preconditioner call: sqrt(g . g) <= tol or it >= max_iter, g . g = the sum of the residual update's
// block partials (sum_partials_wave: the bits of sum_partials).  Every workgroup of that kernel evaluates it for itself and returns at once when it holds; workgroup 0 stores
// PcgScalars::stop, which the later kernels of the call test with `done` and `finishing` and from which the direction update takes its finishing branch - one decision per
// iteration, so a z that was not computed is never read.  gg_part == null: no test here (the direction update decides, behind the preconditioner)
// Whoever runs the test (workgroup 0) also stores the sum in PcgScalars::gg.  per_wave: every wave adds up all the partials for itself even where the kernel could share the
// sum out over its four waves (device_reduce.hpp; A/B hook PORO_PCG_STOP_PER_WAVE).  The word sits in the tail padding: the size of the struct, and with it the layout of the
// kernel arguments that embed it, is what it was.
struct PcgStopTest { PcgScalars *sc = nullptr; const double *gg_part = nullptr; int it = 0; int per_wave = 0; };
static_assert(sizeof(PcgStopTest) == 24, "PcgStopTest is embedded in kernel arguments");

// Mailbox in pinned, device-visible host memory: a one-block kernel at the end of an enqueued sequence copies a few scalars (and optionally the PCG state) into it and
// then raises `seq` with a system-scope release; the host spins on `seq` instead of issuing a device-to-host copy + stream synchronisation (which idled the GPU
// for 20-60 us per round trip, 25 times per time step: profiles/r02_gpu_idle_gaps.txt).
struct Mailbox { volatile unsigned long long seq; unsigned long long pad_; double vals[16]; PcgScalars sc; };

// device-side state of the single-reduction PCG (partitioned runs)
struct Cg1State { double gamma_old, alpha_old, alpha, beta, tol, res0, res; int32_t it, done, converged, pad_; };

// INVERSE Jacobi diagonal handed to the PCG kernels (they multiply): the full vector of reciprocals, or (uniform boxes) a class byte
// per node + table[class][component] of reciprocals
// reciprocal Jacobi diagonal; a ZERO entry marks an inert (Dirichlet) dof that PCG leaves alone (the drivers carry the same set as a byte mask beside it)
struct DiagVec { const double *full = nullptr; const uint8_t *cls = nullptr; const double *tab = nullptr; int ncomp = 1; };

struct FeTablesDev {   // device copies of poro_fe_tables
  int nq_u, nq_p, nq_f, ns_u, ns_p;
  const double *w_qu, *w_qp, *w_qf, *u_qu, *du_qu, *du_qp, *q1_qu, *dq1_qu, *q1_qp, *dq1_qp, *u_qf, *dq1_qf;
};

// uniform-box coupling operator (kernels_box.hip): 1D local blocks N[s][t] = int phi_s psi_t, D[s][t] = int phi_s' psi_t on the unit interval
struct BoxCoupling { int k; int n[3]; double h[3]; double N[3][2], D[3][2]; };

// fast diagonalisation (kernels_fdm.hip): per direction the generalised eigenvectors S (n x n row-major, columns M-orthonormal), S^T, eigenvalues
struct FdmDir { int n = 0; DevBuf<double> S, St, lam; };
struct FdmScalar { int dim = 0; FdmDir dir[3]; bool built = false; };
struct FdmScale { const double *lam[3]; int n[3]; double a, k[3]; int64_t ncol, col0, col_total; };   // divide by a + k0 lam0[i] + k1 lam1[j] + k2 lam2[k] at grid node (i, j, k); ncol > 0: column-distributed layout
// partitioned (slab) form: the transforms of the leading directions are local, the last direction runs on columns gathered by an all-to-all
struct FdmWindow { int n_planes; int64_t ncols_valid, grid_col0, grid_plane0; };   // one peer's share of a window copy (fdm_window_batch)
// what every rank of a slab partition knows about all slabs (ctx_prec.hip: slab_layout), in node planes of the space it was filled for (Q1, or the displacement space)
struct SlabLayout {
  int n_ranks = 1, rank = 0;
  std::vector<int> layers, off;                 // cell layers and first global node plane of every rank
  int ng = 0;                                   // global node planes of the last direction
  int64_t ncol_total = 0, C = 0;                // columns (nodes of one plane) and columns per rank
  int max_own = 0, max_nl = 0;                  // padded plane counts of the two exchanges
};
struct FdmDist : SlabLayout {
  bool built = false;
  FdmDir last;                                  // global eigenvectors of the last direction
  DevBuf<double> sendbuf, recvbuf, tz1, tz2; std::vector<double> hsend, hrecv;
  DevBuf<FdmWindow> windows;                    // [4][n_ranks]: the per-peer windows of the four copies around the two all-to-alls (one launch each)
};

// block fast diagonalisation of the displacement system (kernels_fdmu.hip): per (component, direction) the transform matrices S^T (fwd) and
// S (bwd) in MFMA fragment order and the eigenvalues (inf marks removed modes); coef[c][d] = lambda + 2G (d == c) | G
struct FdmuDir { int n = 0; bool reg_form = false, split = false, blk = false; int n_even = 0; int blk_kk[2] = {0, 0}, blk_nch[2] = {0, 0}, blk_mb[2] = {0, 0} /* [forward, backward] */; DevBuf<double> fwd, bwd, lam; };
struct FdmU : SlabLayout {
              int dim = 0; int nn[3] = {1, 1, 1}; double coef[3][3] = {}; FdmuDir dir[3][3]; FdmuDir last_global[3]; bool built = false, single = false;
              int fix[3][3][2] = {};
              // slab-partitioned form: node planes of the last direction are gathered per column group by an all-to-all (as FdmDist for the Q1 systems)
              bool dist = false; DevBuf<double> sendbuf, recvbuf, tz1, tz2;
              // per-cell moduli (poro_ctx::mod): the last direction is a banded line solve between stage 0 and stage 1 of fdmu_apply (kernels_fdmu_line.hip).  line_coef:
              // [component][3 matrices][k_u + 1 bands][nodes of the line], line_fac: the cached factorisation, (k_u + 1) n_u doubles; both go with the tables (release_fdm_u)
              bool line = false; DevBuf<double> line_coef, line_fac; };
// octant form of the block fast diagonalisation (kernels_fdmo.hip; 3D boxes, one rank, every direction mirror-symmetric for every component).
// The even / odd butterflies of the three directions commute with everything inside the preconditioner, so they are hoisted out of it: the CG residual g and
// the preconditioned residual z live as 8 octants per component, Q[c][o][kz][ky][kx] with o = 4 pz + 2 py + px (p = 0: even part e_k = v_k + v_k', 1: odd
// part o_k = v_k - v_k' of the pair k < h, k' = n - 1 - k; the centre node of an odd line is its own mirror: e = v, o = 0), h = (n + 1) / 2 entries per
// direction.  Each of the 24 (component, octant) blocks is then an independent half-size 3D transform, done in three passes (x y fused per plane, z
// forward + eigenvalue scaling + z backward, y x fused per plane); the butterflies ride in the CG update kernels, which touch every entry anyway.
struct FdmoPlans;
// strip form of the scalar Q1 passes: the share of the CUs a block-per-workgroup launch must reach to keep the block form.  Measured on one MI355X (256 CUs) with
// tools/q1_strips_bench.py, block -> strip form in us per three passes, at (workgroups of the block form) / CUs: 0.09 (24^3 vertices, 1 right-hand side) 24.0 -> 22.6,
// 0.19 (48^3, 1) 32.7 -> 21.7, 0.28 (72^3, 1) 58.1 -> 41.3 and (24^3, 3) 19.0 -> 14.8, 0.56 (48^3, 3) 31.2 -> 23.8 - but 0.47 (120^3, 1; eight tiles) 134.4 -> 140.3,
// 0.84 (72^3, 3) 57.7 -> 71.8, 1.41 (120^3, 3) 265 -> 360: every strip workgroup stages the whole block, so the form pays only while the chip is mostly empty.  The
// crossover lies between 0.28 and 0.47 ("Strip form of the Q1 passes")
constexpr double kFdmoStripFill = 0.4;
struct FdmOct {
  bool built = false; int nt = 0;                 // 16-wide MFMA tiles per half line (max over the directions), 1..8
  int n[3] = {1, 1, 1}, h[3] = {1, 1, 1}; int hxp = 2;   // hxp: row pitch = h[0] rounded up to even (16-byte aligned rows; the pad entry is zero and stays zero)
  int64_t co_stride = 0, n_oct = 0;               // entries per (component, octant) = hxp h[1] h[2]; 24 co_stride
  double coef[3][3] = {};
  DevBuf<double> fwd[3][3][2], bwd[3][3][2], lam[3][3][2];   // [component][direction][parity]: half-size transforms in MFMA fragment order [tile][4 nt][64], eigenvalues (inf = no such mode)
  DevBuf<float> fwd32[3][3][2], bwd32[3][3][2];   // single-rank octant form: the same fragments rounded to fp32 (PORO_FDM_FP32; bwd32 is the exact transpose of fwd32)
  DevBuf<double> g, z, t;                         // residual, preconditioned residual, scratch - all in octant form (PORO_FDM_FP32: t holds the intermediate array as floats, half of it used)
  DevBuf<double> gz_part; int gz_n = 0;           // octant form on one rank: per-workgroup partial sums of g . z left by transform pass 2 (one slot per workgroup of that launch)
  std::vector<double> h_lam[3][3][2];             // host copies of the eigenvalues
  DevBuf<double> bxy;                             // [component][py][px][my][mx] = coef_x lam_x[mx] + coef_y lam_y[my]: the part of the eigenvalue sum a z line shares (pass 2 reads it per column)
  // slab-partitioned form ("quadrant form"): only x and y are split into parities in the CG vectors, Q[c][q = 2 py + px][kz local][ky][kx] (no = 4 blocks per component);
  // the z transform runs on whole global lines after an all-to-all of column chunks, where the z butterfly is applied on the way in / out of the transposed array
  int no = 8;                                     // blocks per component in g, z, t: 8 octants, or 4 quadrants when z is not split locally
  int nc = 3;                                     // components per node: 3; 2 for the planar (2D) form, which is the quadrant form with a single plane
  bool planar = false;                            // 2D: the transforms are batched tiled GEMMs over whole (component, quadrant) planes (fwd = row-major h x h matrices F[mode][node])
  int own_z = 0;                                  // local node planes that count in dot products (the upper shared plane belongs to the neighbour)
  // per-direction form (fdmo_init_per_direction; one rank, 3D, opt-in): only the directions of split_mask (bit d) are split in parities, the others keep whole lines (h[d] = n[d]);
  // no = 2^(split directions) parts per component, Q[c][part][kz][ky][kx] with the parity bits of the split directions packed in the order x, y, z; even row pitch always.
  // nt_z: tiles of pass 2 (the z line), nt those of passes 1 / 3 (x-y planes); every other form has nt_z = nt
  bool per_dir = false; int split_mask = 7, nt_z = 0;
  struct Slab {
    bool on = false; int n_ranks = 1, rank = 0;
    int ng = 0, hzg = 0;                          // global nodes of a z line / rows of a transposed block (half length with the parity split, ng without)
    bool zboth = false; DevBuf<int64_t> dst2;      // z stage with both parity parts of a line per workgroup (no transposed array, no scatter kernel): [ng][2] target offsets of every global plane
    int np = 2, nb = 12;                          // parity parts of the z direction (2; scalar Q1 systems: 1 = no butterfly), blocks of the local arrays (3 components x 4 quadrants; scalar: 1)
    int cw = 64, nchunk = 0, cps = 0, chunk0 = 0, my_chunks = 0;   // chunk width (columns), chunks per (component, quadrant) plane, chunks per rank share, this rank's first global chunk and count
    int64_t scols = 0;                            // columns of a share = cps cw
    int own = 0, nl = 0, max_own = 0, max_nl = 0, rows_back = 0;    // planes this rank sends (owns) / holds; maxima over the ranks; sum of the ranks' local planes
    int64_t recv_off = 0;                         // buf = [send | recv], each [rank][plane][scols]; a rank's own block is written straight into the receive half
    DevBuf<int64_t> row_in;                       // [ng]: offset (in buf) of global plane kz after the gathering all-to-all
    DevBuf<int64_t> row_out; DevBuf<int32_t> row_kz;   // [rows_back]: offset (in buf) of a row of the scattering all-to-all, global plane of that row
    DevBuf<double> buf, tz;                       // all-to-all buffers; transposed array [chunk][pz][hzg][cw]
  } slab;
  // class-split passes (single-rank octant form, fp64; fdmo_upload_dir_classes): every (component, direction) line passed class_split_tables.  Per [component][direction][parity]:
  // the two class transforms [class: vertex, midpoint] in fragment order, the mixes [64 slots][4], the eigenvalues by slot [class][64]; bxy_vm = bxy in the class-major mode order
  bool class_split = false;
  DevBuf<double> cfwd[3][3][2][2], cbwd[3][3][2][2], cmix[3][3][2], clam[3][3][2], bxy_vm; std::vector<double> h_clam[3][3][2];
  std::shared_ptr<FdmoPlans> plans;              // displacement forms: the launch descriptors of the three passes, planned once by fdmo_finalize (kernels_fdmo.hip)
  struct ScalarTable { double a, kappa; DevBuf<double> t; };
  std::list<ScalarTable> scalar_tables;           // scalar form: a + kappa (lam_x + lam_y) per plane position, one table per (a, kappa) seen (pressure Jacobian, mass matrix)
  // scalar form on one rank: a pass whose block-per-workgroup launch would start fewer workgroups than this runs in the strip form (k_fdmo_strip, fdmo_scalar_apply_many);
  // kFdmoStripFill x the CUs of the device, set where the table set is built (PORO_FDMO_SCALAR_STRIPS = another factor; 0 keeps every pass in the block form)
  double strip_limit = 0;
};
// one table set of the scalar Q1 systems: the six-launch form (kernels_fdm.hip) and, where usable, the same tables for the three-launch transform kernel
// (kernels_fdmo.hip: 3D boxes, lines of at most 80 vertices)
struct FdmQ1 { FdmScalar nodal; FdmOct fused; };
// dependency levels of the lower / upper triangle in natural row order (rows of one level can be swept concurrently)
struct SsorLevels { DevBuf<int32_t> fwd_rows, bwd_rows; std::vector<int64_t> fwd_off, bwd_off; bool built = false; };
struct CsrDev {
  int64_t n = 0, nnz = 0;
  DevBuf<int64_t> rp; DevBuf<int32_t> col; DevBuf<int64_t> diag_pos;
  int lanes_per_row = 8;
  SsorLevels ssor;
};

// closed affine constraints (hanging nodes) on the device: forward lists (constrained dof -> masters) for expand / distribute and the
// transposed lists (master -> constrained dofs) so that the reduction C^T y is a gather without atomics
struct ConsDev {
  int64_t n = 0, n_masters = 0;
  DevBuf<int32_t> dof, master; DevBuf<int64_t> ptr; DevBuf<double> weight, inhom;
  DevBuf<int32_t> t_master, t_dof; DevBuf<int64_t> t_ptr; DevBuf<double> t_weight;
  DevBuf<uint8_t> inert;   // byte mask: constrained (Dirichlet or hanging) dofs stay out of the Krylov system
  DevBuf<uint8_t> hanging; // pressure space with both lists only: the hanging dofs alone (the projection's mass matrix has no prescribed rows)
  bool any_inhom = false;
};

struct Timer { double seconds = 0; int64_t launches = 0 /* with events */, enqueued = 0 /* all */; std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
               bool sample(int stride) { return enqueued++ % stride == 0; } };

// interface of a general partition in one dof space (poro_partition.shared_*): concatenated per-neighbour lists for packing / receiving, and per
// shared dof the sources of its sum in ascending rank order (-1 = this rank's own partial value, otherwise a position in `recv`)
struct IfcDev {
  int64_t m_send = 0, m_shared = 0, n_owned = 0;
  std::vector<int64_t> ptr;                 // [n_neighbours + 1] into dof / send / recv
  DevBuf<int32_t> dof, sh_dof, sh_src; DevBuf<int64_t> sh_ptr; DevBuf<double> send, recv;
  std::vector<double> hsend, hrecv;         // host staging of the callback communicator
};

struct Comm {
  poro_partition part{};
  bool general = false; std::vector<int32_t> neighbours; IfcDev ifc_u, ifc_p;
  // RCCL (resolved at run time from librccl.so.1)
  void *nccl_comm = nullptr;
  // host-staged callbacks (tests)
  poro_allreduce_fn ar = nullptr; poro_sendrecv_fn sr = nullptr; void *user = nullptr;
  DevBuf<double> recv_lo, recv_hi; std::vector<double> hsend, hrecv;
  // pinned host staging of vector all-reduces through the callbacks (allreduce_sum_vec), grown on demand
  struct Pinned { double *p = nullptr; size_t n = 0; Pinned() = default; Pinned(const Pinned &) = delete; Pinned &operator=(const Pinned &) = delete; ~Pinned() { if (p) (void)hipHostFree(p); } } hvec;
  bool force_multi = false;
  bool multi() const { return part.n_ranks > 1 || force_multi; }
};

// face tables of the Kelly error indicator (ctx_adapt.hip), built at the first poro_pres_estimate_error: interior (sub)faces sorted by their first cell, and per cell
// the list of its faces with the cell whose diameter scales them
struct KellyDev { bool built = false; int64_t n_faces = 0; DevBuf<int32_t> cell_a, cell_b, code, ent_face, ent_hcell; DevBuf<int64_t> ent_ptr; DevBuf<double> jump, eta; };

// hybrid operator form on refined boxes (poro_ctx_set_operator_form; kernels_hyb.hip, ctx_hybrid.hip): everything derived on the host at the first enable
struct HybridPlan {
  bool built = false;
  int64_t n_box_nodes = 0, n_fine_cells = 0, n_removed = 0, n_chunks = 0;
  DevBuf<int64_t> inj;                                            // [box node] -> mesh node
  DevBuf<int32_t> color_cells; std::vector<int64_t> color_off;    // the context's colour classes restricted to the fine cells (offsets from 0)
  DevBuf<int32_t> spatial_cells;                                  // the fine cells in the Morton order of the atomic scatter mode
  DevBuf<int32_t> removed_cells, slot;                            // the refined box cells; [box cell] -> its position in that list or -1
  DevBuf<uint8_t> touched;                                        // [box node]: belongs to a refined cell (handled by the listed-node kernel)
  DevBuf<double> Ke_t, V;                                         // the box's element matrix transposed; slab [refined cell][dofs per cell] of Ke x_box|_c
  DevBuf<int64_t> nodes; DevBuf<int32_t> chunk_cls;               // the touched nodes sorted by position class, every class padded with -1 to whole waves; class of every 64-node chunk
  DevBuf<double> x_box, y_box;                                    // box-sized work vectors of the plan (the box context's own belong to the two-level preconditioner)
};

struct BoxDev { int enabled = 0; int n[3] = {1, 1, 1}; int nn[3] = {1, 1, 1}; double h[3] = {1, 1, 1}; };

}  // namespace poro

struct poro_ctx {
  poro_ctx() = default; poro_ctx(const poro_ctx &) = delete; poro_ctx &operator=(const poro_ctx &) = delete;
  ~poro_ctx() { if (mailbox) (void)hipHostFree(mailbox); }
  int device = 0, operator_mode = PORO_OP_CSR;
  hipStream_t stream = nullptr;
  int dim = 2, k_u = 2, ns_u = 9, ns_p = 4, dpc_u = 18, dpc_p = 4, nv = 4;
  int64_t n_cells = 0, n_u = 0, n_p = 0;
  poro_material mat{};
  poro::BoxDev box;
  // the logical tensor structure the fast-diagonalisation preconditioners work on: the uniform box, or a tensor-product grid without the box tag (poro_desc.tensor)
  struct Lines { bool on = false, uniform = true; int n[3] = {1, 1, 1}, nn[3] = {1, 1, 1}; std::vector<double> hcell[3]; } lines;
  poro::Comm comm;
  // mesh / dof data
  poro::DevBuf<int32_t> cell_dofs_u, cell_dofs_p, color_cells;
  poro::DevBuf<double> cell_X, tables;
  poro::DevBuf<double> cell_geo;          // 3D meshes whose cells are all parallelepipeds: J^-1 (9, row-major [b][d] = d xi_b / d x_d) and det J per cell (kernels_mfg.hip)
  poro::FeTablesDev fe{};
  int mfg_sf = 0;                            // poro_desc.fe holds the Gauss(k+1) / equidistant-Lagrange tables the sum-factorised general kernels hard-code (kernels_mfg.hip)
  std::vector<int64_t> color_off;            // host offsets into color_cells
  // scatter mode of the general cell-loop operator (poro_ctx_set_scatter_mode).  spatial_cells: all cells in Morton order of their centroids, built the first time the
  // context enters the atomic mode
  int scatter_mode = 0; poro::DevBuf<int32_t> spatial_cells;
  // operator form of the general matrix-free operator (poro_ctx_set_operator_form): PORO_OPFORM_GENERAL, or the hybrid of the box's structured kernel and the fine cells
  int operator_form = 0; poro::HybridPlan hyb;
  // transform precision of the displacement system's block FDM where it runs in the single-rank 3D octant form (poro_ctx_set_fdm_precision); every other form ignores it
  int fdm_precision = 0;
  // form of the displacement system's block FDM (poro_ctx_set_fdm_form): PORO_FDM_FORM_PER_DIRECTION is honoured by single-rank 3D contexts only; fdm_form_fixed: the nested
  // coarse box of a two-level preconditioner, which keeps the default whatever is asked
  int fdm_form = 0; bool fdm_form_fixed = false;
  poro::DevBuf<uint8_t> dir_mask, node_mask; poro::DevBuf<double> dir_val; poro::DevBuf<int32_t> dir_dofs;
  std::vector<int32_t> h_dir_dof; std::vector<double> h_dir_val;
  poro::ConsDev cons_u, cons_p;
  poro::DevBuf<uint8_t> pdir_mask; poro::DevBuf<double> pdir_val; int64_t n_pdir = 0;   // extension: prescribed pressures
  // the prescribed set is exactly a union of whole faces (direction, side) of `lines` (face analysis at set-up): deleting those rows and columns leaves a Kronecker sum of
  // 1D matrices without their end nodes, which the table set q1_fixed below diagonalises
  bool pdir_faces_ok = false; int pdir_face[3][2] = {{0, 0}, {0, 0}, {0, 0}};
  poro::DevBuf<int32_t> bface_cell, bface_local, bface_id, neu_label, neu_comp; poro::DevBuf<double> neu_val;
  poro::DevBuf<int32_t> bface_order; std::vector<int64_t> bface_group_off;   // boundary faces sorted by (colour of the cell, local face): the groups of asm_u_neumann
  int64_t n_bfaces = 0; int n_neumann = 0;
  // matrices
  poro::CsrDev Ap, Au;                       // pressure pattern (mass, Laplace, Jacobian share it), displacement pattern
  poro::DevBuf<double> Mp, Kp, Jp, Au_val;
  bool projection_matrix_ready = false;
  poro::DevBuf<double> Ke;                   // reference element matrix of the matrix-free operator
  // vectors (ids of include/poroel_hip.h)
  std::map<int, poro::DevBuf<double>> vec, vec_saved;
  poro::DevBuf<uint8_t> rhs_u_flags;   // box_rhs_u_flags of lift_u and neumann_u, rebuilt with them (box_asm only)
  poro::DevBuf<double> lift_u, neumann_u, diag_u, diag_u_local, diag_J, diag_M, src_local;
  poro::DevBuf<double> dinv_u, dinv_J, dinv_M;   // reciprocals of the Jacobi diagonals
  poro::DevBuf<uint8_t> diag_u_cls; poro::DevBuf<double> diag_u_tab;   // dictionary form of diag_u (uniform boxes): class per node + table[class][dim]
  poro::DevBuf<double> wg_u, wd_u, wh_u, wg_p, wd_p, wh_p, tmp_p, proj_y;
  bool box_asm_checked = false;
  int box_asm = 0 /* 0 off, 1 unchecked, 2 checked against the per-cell kernels */; poro::BoxCoupling box_cpl{};
  poro::DevBuf<double> ilu_u, ilu_J, ilu_M; bool ilu_u_valid = false, ilu_J_valid = false, ilu_M_valid = false;   // ILU(0) factors on the CSR patterns
  poro::DevBuf<double> wz_p;   // z = P^-1 g of an explicit preconditioner (pressure-sized systems)
  // fast diagonalisation of the Q1 box operators, two table sets (ctx_prec.hip: build_fdm_q1).  q1_free: a M + kappa K on the whole grid - the projection mass matrix,
  // the pressure Jacobian without prescribed rows; slab partitions (fdm_dist) use this set alone.  q1_fixed: the pressure Jacobian with the prescribed faces' end nodes
  // removed (built only when n_pdir != 0, one rank).  fdm_t1 / fdm_t2 are shared
  poro::FdmQ1 q1_free, q1_fixed; poro::FdmDist fdm_dist; poro::DevBuf<double> fdm_t1, fdm_t2;
  double cheb_lmax = 0;   // estimate of lambda_max(D^-1 A_u) (Lanczos at matrix build; 0 = not yet computed)
  double cheb_ratio_default = 0;   // default interval ratio of the Chebyshev preconditioner, from the GLOBAL mesh size (0 = not yet computed)
  poro::DevBuf<double> cheb_z, cheb_t;
  poro::FdmOct fdm_oct;
  // two-level preconditioner (poro_desc.coarse): the underlying uniform box as a context of its own (same device and stream) + the node-wise interpolation P and its transpose
  struct Interp { int64_t n_fine = 0, n_coarse = 0; int lanes = 1, lanes_t = 1;   /* lanes per row of the interpolation kernels, from the mean row length */ poro::DevBuf<int64_t> p_ptr, pt_ptr; poro::DevBuf<int32_t> p_col, pt_col; poro::DevBuf<double> p_w, pt_w; };   // P (rows = fine) and its transpose as CSR
  struct TwoLevel : Interp { poro_ctx *box = nullptr; Interp pressure; bool pdir_nested = false; /* prescribed pressures: every fine dof on a prescribed coarse dof is prescribed */ } two_level;   // (the base part: displacement nodes; .pressure: pressure dofs, optional)
  bool borrowed_stream = false;     // (the box context of a two-level preconditioner runs on its parent's stream)
  poro::FdmU fdm_u; poro::DevBuf<double> fdmu_t1, fdmu_t2, wz_u; int fdm_u_state = 0 /* 0 unknown, 1 usable, -1 not separable */; std::string fdm_u_why;
  std::vector<uint8_t> h_node_mask;
  poro::DevBuf<double> partials; poro::DevBuf<poro::PcgScalars> scal; poro::DevBuf<double> red;   // red: kScalarSlots doubles
  poro::Mailbox *mailbox = nullptr; unsigned long long mb_seq = 0;   // pinned host memory (hipHostMalloc), device-visible at the same address
  int timing_stride = 1;   // events on every timing_stride-th launch of a family (poro_timers_enable)
  poro::DevBuf<double> cheb_side_lo, cheb_side_hi;   // partial products of the fused Chebyshev kernel on the shared planes (slab partitions)
  poro::DevBuf<poro::Cg1State> cg1_state; poro::DevBuf<double> cg1_z[2], cg1_w[2];   // single-reduction PCG of partitioned runs ([0]: displacement-sized, [1]: pressure-sized)
  bool matrix_built = false;
  int interleaved_u = 0;
  int pcg_hint_fdm_u[2] = {0, 0}, pcg_hint_cheb_u[2] = {0, 0}; int64_t cheb_applies = 0;
  int pcg_hint_u[2] = {0, 0};   // iterations of the last two displacement solves (batch scheduling of the next one)
  int pcg_hint_p[2] = {0, 0}, pcg_hint_proj[2] = {0, 0};   // the same for the iterative pressure / projection solves
  int n_cus = 256; int mf_variant = 1 /* 0 element-matrix gather, 1 sum-factorised (where supported) */; int mask_anywhere = 0;
  // timing
  bool timing = false; std::map<std::string, poro::Timer> timers; std::vector<hipEvent_t> event_pool;
  double jac_dt = -1;
  // the pressure Newton loop (ctx_pressure.hip): pres_host_loop = PORO_PRES_HOST_LOOP was set when the context was made (the per-call loop, A/B hook); the gate and the record of a
  // batch; per call slot of a time step the residual evaluations that call took last time (0 = unknown; cleared by poro_state_restore like the iteration-count hints)
  bool pres_host_loop = false; poro::DevBuf<poro::PcgScalars> newton_gate; poro::DevBuf<double> newton_rec; int newton_hint[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  poro::KellyDev kelly;
  // The per-cell coefficient fields (ctx_fields.hip; one rank).  Both are a poro::CellField (cell_field.hpp): kind 0 none, 1 layered along the slowest direction of
  // `lines`, 2 general; host[a]: the caller's arrays; layer[a]: per cell layer of that direction the value (kind 1) or the arithmetic mean (kind 2) - the coefficients of
  // the line-solve forms of PORO_PREC_FDM.  What each adds is its device state.  perm: k / mu of the pressure system, components 0 .. ncomp - 1.  ncomp: 0 while
  // kind == 0, 1 for one k / mu per cell (poro_ctx_set_cell_permeability), dim for the diagonal tensor diag(kx, ky[, kz]) / mu (poro_ctx_set_cell_permeability_tensor).
  // cell: [n_cells][ncomp] in the caller's cell order (the weights of the assembly, Kp = K_kappa).  lattice: one plane of n_cells per component, each in lattice cell
  // order (consecutive lanes of the stencil kernels of matrix-free boxes read consecutive addresses).  line: one set of 1D arrays (perm_line_coefficients) and cached
  // reciprocal pivots per table set (free ends / fixed ends); `a` = the 1 / (M_b dt) the pivots belong to
  struct Perm : poro::CellField<3> {
    int ncomp = 0;
    poro::DevBuf<double> cell, lattice;
    struct Line { bool built = false; int lo = 0, hi = 0; double a = -1; poro::DevBuf<double> coef, inv; } line[2];
  } perm;
  // mod: (Lame lambda, shear modulus G) of the displacement system, components 0 and 1.  cell: [n_cells][2] = (lambda, G) in the caller's cell order, what the general
  // cell kernels and the coloured assembly read.  node: [n_p][2], the arithmetic mean over the cells that touch a pressure dof - the constants of the effective stresses and
  // of the fixed-stress strain update.  While kind != 0 a box-tagged context runs the general cell loop for everything that depends on the moduli (box_fast_u below)
  // planes: the per-plane weight table of the structured operator for layered moduli (moduli_planes.hpp), uploaded while that form is effective (moduli_structured below)
  struct Moduli : poro::CellField<2> { poro::DevBuf<double> cell, node, planes; } mod;
  // requested form of the displacement operator on a box with per-cell moduli (poro_ctx_set_moduli_operator): PORO_MODULI_OP_CELLS, the general cell loop, or
  // PORO_MODULI_OP_STRUCTURED, kernels_kron_lm.hip where it applies.  Never chosen automatically; stays through field changes
  int moduli_op = 0;
  // Gravity (poro_ctx_set_gravity, poro_ctx_set_cell_density; ctx_fields.hip, kernels_gravity.hip).  on: g has a non-zero component.  dens: the per-cell bulk density
  // (one rank), cell: [n_cells] in the caller's cell order, lattice: the same in lattice cell order (uniform boxes); kind 0: the scalar rho_b.  body_u / flux_p: the two
  // gravity vectors alone (rank-partial sums on a partition), built while gravity is on.  They are folded into constant vectors the step kernels read anyway: body_u is
  // summed into neumann_u behind the tractions (assemble_loads_u), src_p = src_local + flux_p takes the place of src_local in the pressure residual (source_p below) -
  // src_local and PORO_VEC_SOURCE_P keep meaning the well alone.  loads_stale: neumann_u and rhs_u_flags have to be rebuilt before the next right-hand side
  struct Gravity {
    bool on = false, loads_stale = false; double g[3] = {0, 0, 0}, rho_b = 0, rho_f = 0;
    struct Density : poro::CellField<1> { poro::DevBuf<double> cell, lattice; } dens;
    poro::DevBuf<double> body_u, flux_p, src_p;
    bool flux_on() const { return on && rho_f != 0; }
  } grav;
  // Flow post-processing (ctx_flux.hip, kernels_darcy.hip), allocated at the first call: q [n_cells][dim], Qf [n_bfaces], the scratch of the balance (t = the residual's
  // storage term, rt = C^T(-r), out = rt on the prescribed dofs), m = the lumped pressure mass M 1 (built once), pdir_dof = the prescribed dofs in the descriptor's order
  struct Flux { bool built = false; poro::DevBuf<double> q, Qf, Ql, m, t, rt, out, sums; poro::DevBuf<int32_t> labels, pdir_dof; } flux;
  std::vector<int32_t> h_pdir_dof;   // poro_desc.dirichlet_dof_p as given
  // Mechanical post-processing (ctx_stress.hip, kernels_stress.hip), allocated at the first call of each kind: strain / eff / tot [n_cells][n_sym], measures [n_cells][6];
  // the scratch of the force balance (au = A_full u, then Rt; cpl, neu = the coupling and traction vectors on all rows; zero_u / zero_mask = what the box kernel of the
  // coupling takes for lifting, loads and mask; out = Rt on the Dirichlet dofs), comp = the component of every displacement dof (built once)
  struct Stress { bool cells_built = false, balance_built = false; poro::DevBuf<double> strain, eff, tot, measures, summary, partials, au, cpl, neu, zero_u, out, sums;
                  poro::DevBuf<uint8_t> comp, zero_mask; } stress;
};

namespace poro {

// the constant-coefficient structured kernels (k_kron*, the single Ke, box_asm_u_matrix, the diagonal dictionary) serve the displacement system: a box without per-cell moduli
inline bool box_fast_u(const poro_ctx *c) { return c->box.enabled && !c->mod.kind; }
// where the structured operator for layered moduli can stand in for the cell loop: a single-rank uniform 3D box of degree 1 or 2 in matrix-free mode with the
// sum-factorised variant, and a field that is constant within every cell layer of z
inline bool moduli_structured_applies(const poro_ctx *c) {
  return c->box.enabled && c->dim == 3 && (c->k_u == 1 || c->k_u == 2) && c->mod.kind == 1 && c->operator_mode == PORO_OP_MATRIX_FREE && c->mf_variant == 1 && !c->comm.multi() &&
         c->comm.part.n_ranks <= 1;
}
// ... and does: requested, and the table is on the device (ctx_fields.hip: sync_moduli_planes keeps the two in step)
inline bool moduli_structured(const poro_ctx *c) { return c->moduli_op == PORO_MODULI_OP_STRUCTURED && c->mod.planes.p && moduli_structured_applies(c); }

// ---- kernels_la.hip -----------------------------------------------------------------------------
void la_fill(hipStream_t s, double *x, double v, int64_t n);
// copy n <= 16 doubles from `src` (device) and optionally *sc into the host mailbox, then publish sequence number `seq` (system-scope release)
// node-wise sparse interpolation of a node-interleaved vector: out[(row, c)] = sum_k w[k] in[(col[k], c)] (prolongation by P, restriction by its transpose)
void la_nodal_interp(hipStream_t s, const int64_t *ptr, const int32_t *col, const double *w, int64_t n_rows, int ncomp, const double *in, double *out, int lanes = 1);
// z = omega D^-1 g + P z_c, zero on the inert dofs (additive two-level preconditioner)
void la_two_level_combine(hipStream_t s, const int64_t *ptr, const int32_t *col, const double *w, int64_t n_rows, int ncomp, const double *zc, const double *g, const double *dinv, const uint8_t *inert, double omega, double *z, int lanes = 1);
void la_copy_many(hipStream_t s, int count, double *const *dst, const double *const *src, const int64_t *n);   // several device-to-device copies in one launch
void la_post(hipStream_t s, Mailbox *mb, unsigned long long seq, const double *src, int n, const PcgScalars *sc);
void la_reduce_post(hipStream_t s, const double *partials, int n_sets, double *red, int max_not_sum_mask, Mailbox *mb, unsigned long long seq);   // la_reduce_finish + la_post(red, n_sets) in one launch
void la_copy(hipStream_t s, double *y, const double *x, int64_t n);
void la_axpy(hipStream_t s, double *y, double a, const double *x, int64_t n);
void la_add_range(hipStream_t s, double *y, const double *x, int64_t n);
// the pressure Newton loop as a gated batch (poro_pres_newton_loop): gate->done != 0 makes every one of these but la_newton_reset / la_newton_post a no-op
void la_axpy_gated(hipStream_t s, double *y, double a, const double *x, int64_t n, const PcgScalars *gate);
void la_newton_update(hipStream_t s, double *p, double *ev, double c, const double *dp, int64_t n, const PcgScalars *gate);      // p += dp, ev += c dp
void la_newton_reset(hipStream_t s, PcgScalars *gate, double *rec /*[kNewtonRecord]*/);
void la_newton_residual_test(hipStream_t s, const double *partials, double tol, int slot, PcgScalars *gate, double *rec);
void la_newton_check_test(hipStream_t s, const double *partials /*[2 kMaxPartials]*/, double abs_tol, double rel_tol, int slot, PcgScalars *gate, double *rec);
void la_newton_post(hipStream_t s, const double *partials_inf, double *rec, Mailbox *mb, unsigned long long seq);
void la_add_two_ranges(hipStream_t s, double *y0, const double *x0, double *y1, const double *x1, int64_t n);
// partials-based reductions; results land in red[slot..] after la_reduce_finish
void la_dot_partials(hipStream_t s, const double *a, const double *b, int64_t n, double *partials /*[kMaxPartials]*/, const PcgScalars *gate = nullptr /* no-op once gate->done / finishing */);
void la_norm_partials(hipStream_t s, const double *a, int64_t n, double *partials_l2, double *partials_inf);
void la_reduce_finish(hipStream_t s, const double *partials, int n_sets, double *red /*[n_sets]*/, int max_not_sum_mask);
void la_csr_spmv(hipStream_t s, const CsrDev &A, const double *val, const double *x, double *y);
// R = -(M t + kappa K p + src)
void la_csr_residual(hipStream_t s, const CsrDev &A, const double *M, const double *K, double kappa, const double *t, const double *p,
                     const double *src, double *R);
void la_pressure_tmp(hipStream_t s, double *t, const double *ev, const double *ev0, const double *p, const double *p_old, double c1, double c2, int64_t n, const PcgScalars *gate = nullptr);
void la_jacobian(hipStream_t s, double *J, const double *M, const double *K, double a, double kappa, int64_t nnz);
void la_ifc_pack(hipStream_t s, const IfcDev &I, const double *v);
void la_ifc_sum(hipStream_t s, const IfcDev &I, double *v);
void la_csr_diag(hipStream_t s, const CsrDev &A, const double *val, double *diag);
void la_reciprocal(hipStream_t s, double *y, const double *x, int64_t n);
void la_pointwise_mul(hipStream_t s, double *y, const double *x, int64_t n);   // y *= x
// polynomial preconditioner in root form around the (inverse) Jacobi diagonal: z1 = s D^-1 g;  z_new = z_j + omega D^-1 (g - A z_j);
// gz_partials != nullptr: block partials of g . z_new over the first n_owned entries
void la_cheb_first(hipStream_t s, double *z, const double *g, const DiagVec &dv, double scale, int64_t n);
void la_cheb_step(hipStream_t s, double *znew, const double *zj, const double *g, const double *Az, const DiagVec &dv, double omega, int64_t n, int64_t n_owned, double *gz_partials);
// shared planes of a slab partition after the fused kernel: z_{j+1} = z_j + omega D^-1 (g - (own partial + neighbour's partial)) on the first (lo) / last (hi) `plane` dofs of a vector of n
void la_cheb_fix_planes(hipStream_t s, double *znew, const double *zj, const double *g, const double *own_lo, const double *nbr_lo, const double *own_hi, const double *nbr_hi, const DiagVec &dv, double omega, int64_t n, int64_t plane);
// x[dof_i] = sum_k w_k x[master_k] (+ inhomogeneity_i): ConstraintMatrix::distribute; with_inhom = false inside the Krylov iteration
void la_cons_expand(hipStream_t s, const ConsDev &C, double *x, bool with_inhom);
// y <- C^T y: y[master] += sum w y[dof_i], then y[dof_i] = 0 (ConstraintMatrix::condense of a vector)
void la_cons_reduce(hipStream_t s, const ConsDev &C, double *y);
void la_xpby(hipStream_t s, double *y, double a, double b, const double *x, int64_t n);   // y = a y + b x
void la_ilu0_factor(hipStream_t s, const CsrDev &A, const SsorLevels &lv, double *lu /* in: A's values, out: L (unit diagonal) and U */, int *flag /* device int, 0 = ok, else 1 + row of a zero pivot */);
void la_ilu_apply(hipStream_t s, const CsrDev &A, const double *lu, const SsorLevels &lv, const double *src, double *dst);
void la_ssor_apply(hipStream_t s, const CsrDev &A, const double *val, const SsorLevels &lv, double omega, const double *src, double *dst);
void la_sum_strains(hipStream_t s, double *ev, const double *const *strains, int n, int64_t len);
void la_effective_stress(hipStream_t s, const double *const *strains, double *const *stresses, int dim, double lam, double G, int64_t len);
// the same two with nodal constants node_mod[len][2] = (lambda, G): sigma from them; ev[i] += alpha / (lambda_i + 2 G_i / 3) dp[i]
void la_effective_stress_nodal(hipStream_t s, const double *const *strains, double *const *stresses, int dim, const double *node_mod, int64_t len);
void la_strain_update_nodal(hipStream_t s, double *ev, const double *dp, double alpha, const double *node_mod, int64_t len);
void la_set_constrained(hipStream_t s, double *x, const uint8_t *mask, const double *val, int64_t n);
void la_rhs_u_finish(hipStream_t s, double *rhs, const double *lift, const double *neumann, const uint8_t *mask, int64_t n);
// PCG pieces (device-side control, see solver in ctx.hip)
void pcg_init_residual(hipStream_t s, double *g, const double *Ax, const double *b, const uint8_t *inert /*nullable*/, int64_t n);
void la_mask_zero(hipStream_t s, double *x, const uint8_t *mask, int64_t n);
void pcg_dot_dh(hipStream_t s, const PcgScalars *sc, const double *d, const double *h, int64_t n_owned, double *partials);
// z (here and in the two fused updates): the explicit preconditioner's vector z = P^-1 g, null for Jacobi / none (prec)
void pcg_first_direction(hipStream_t s, double *d, const double *g, const DiagVec &diag, const double *z, int prec, int64_t n, int64_t n_owned, double *partials /*2 sets: gg, gz*/);
void pcg_scalars_sum(hipStream_t s, const double *partials, int n_sets, double *red);
void cg1_dots(hipStream_t s, const double *g, const double *z, const double *w, const double *b /*nullable: adds b.b*/, int64_t n_owned, double *partials /*4 sets*/);
void cg1_scalars(hipStream_t s, Cg1State *st, const double *red, int first, double abs_tol, double rel_tol, int max_iter, int stop_rule);
void cg1_update(hipStream_t s, const Cg1State *st, double *d, double *sv, double *x, double *g, const double *z, const double *w, const DiagVec &dv, const uint8_t *inert,
                double *z1_out /* nullable: also store z1_scale D^-1 g_new there */, double z1_scale, int64_t n);
void pcg_scalars_start(hipStream_t s, PcgScalars *sc, const double *red /*bb, gg, gz*/, double abs_tol, double rel_tol, int max_iter, int stop_rule);
// single-rank fast path: the consumers reduce the block partials themselves (no scalar kernels, no host round trip);
// parity = iteration index & 1 selects the g.z slot read / written
void pcg_update_g_fused(hipStream_t s, PcgScalars *sc, int parity, double *g, const double *h, const DiagVec &diag, const double *z, double *z1_out /* as cg1_update */, double z1_scale, int prec, int64_t n, int64_t n_owned,
                        const double *partials_dh, const double *red /*null: single rank*/, double *partials_out /*2 sets*/);
void pcg_update_d_fused(hipStream_t s, PcgScalars *sc, int parity, int it, double *x, double *d, const double *g, const DiagVec &diag, const double *z, int prec, int64_t n,
                        const double *partials_in /*2 sets*/, const double *red /*null: single rank*/);

// ---- kernels_kelly.hip: mesh adaptation (Kelly indicator, transfer of the pressure-space vectors) ----
void kelly_faces(hipStream_t s, int dim, int64_t n_faces, const int32_t *cell_a, const int32_t *cell_b, const int32_t *code, const double *cell_X, const int32_t *cell_dofs_p,
                 const double *p, double *jump);
void kelly_cells(hipStream_t s, int dim, int64_t n_cells, const int64_t *ent_ptr, const int32_t *ent_face, const int32_t *ent_hcell, const double *cell_X, const double *jump, double *eta);
void transfer_rows3(hipStream_t s, int64_t n_rows, const int64_t *ptr, const int32_t *col, const double *w, const double *const in[3], double *const out[3]);

// ---- kernels_darcy.hip: Darcy velocity, boundary discharge, fluid mass balance ----
struct DarcyGravity { double v[3]; };   // rho_f g, zeros unless Gravity::flux_on()
// kappa_c: ncomp = 0 the scalar `kappa`; 1: perm_cell[n_cells]; dim: perm_cell[n_cells][dim] (poro_ctx::Perm::cell)
struct DarcyArgs { int dim, ncomp; int64_t n_cells; const double *cell_X; const int32_t *cell_dofs_p; const double *p; double kappa; const double *perm_cell; DarcyGravity rg; };
void darcy_cells(hipStream_t s, const DarcyArgs &a, double *q /* [n_cells][dim] */);
void darcy_bfaces(hipStream_t s, const DarcyArgs &a, int64_t n_bfaces, const int32_t *bface_cell, const int32_t *bface_local, double *Q /* [n_bfaces] */);
void darcy_label_sums(hipStream_t s, int64_t n_bfaces, const int32_t *bface_id, const double *Q, const int32_t *labels, int32_t n_labels, double *out /* [n_labels] */);
// sums over the n pressure dofs, one slab of kMaxPartials block partials each: 0 m c_strain (ev - ev0), 1 m c_pres (p - p_old), 2 src, 3 Rt on the rows of pdir_mask (nullable),
// 4 Rt on the other rows, 5 Rt^2 on the other rows
struct FlowBalanceArgs { int64_t n; const double *p, *p_old, *ev, *ev0, *m, *src, *Rt; const uint8_t *pdir_mask; double c_strain, c_pres; };
void flow_balance_partials(hipStream_t s, const FlowBalanceArgs &A, double *partials /* [6][kMaxPartials] */);
void darcy_gather(hipStream_t s, int64_t n, const int32_t *idx, const double *src, double *dst);   // dst[i] = src[idx[i]]

// ---- kernels_stress.hip: cell strains and stresses, failure measures, force balance ----
// cell_mod: [n_cells][2] = (lambda, G) or null: lam, G; p null: no pressure (total = effective)
struct StressArgs { int dim, k_u; int64_t n_cells; const double *cell_X; const int32_t *cell_dofs_u, *cell_dofs_p; const double *u, *p; double lam, G, alpha; const double *cell_mod; };
void stress_cells(hipStream_t s, const StressArgs &a, double *strain, double *eff, double *tot /* [n_cells][n_sym] each */);
// measures[n_cells][6] from strain / eff as stress_cells left them; with_mc: also summary[3] = max f, its lowest cell, the number of cells with f >= 0 (through `partials`, 3 slabs)
void stress_measures_cells(hipStream_t s, int dim, int64_t n_cells, const double *strain, const double *eff, double lam0, const double *cell_mod, bool with_mc, double sin_phi,
                           double c_cos_phi, double *measures, double *partials, double *summary);
void dof_components(hipStream_t s, int64_t n_entries, int dim, const int32_t *cell_dofs_u, uint8_t *comp /* [n_u] */);
void force_residual(hipStream_t s, int64_t n, const double *Au, const double *cpl, const double *neu, const double *body /* nullable */, double *r);   // r = A u - (cpl + neu + body)
// sums over the n displacement dofs, one slab of kMaxPartials block partials each: 5 k + {0 Rt on the Dirichlet rows, 1 Rt on the other rows, 2 neu, 3 body (nullable), 4 cpl} of
// component k = comp[i], then 5 dim: Rt^2 on the non-Dirichlet rows
// out[k < dim] = sum over the constraint rows h of component k of (1 - sum of the row's weights) r_h (r BEFORE la_cons_reduce); one block, fixed order
void force_deficit(hipStream_t s, int dim, const ConsDev &C, const double *r, const uint8_t *comp, double *out /* [dim] */);
struct ForceBalanceArgs { int64_t n; const uint8_t *comp, *dir_mask; const double *Rt, *neu, *body, *cpl; };
void force_balance_partials(hipStream_t s, int dim, const ForceBalanceArgs &A, double *partials /* [5 dim + 1][kMaxPartials] */);

// ---- kernels_asm.hip ----------------------------------------------------------------------------
struct AsmArgs {
  int dim, k_u, ns_u, ns_p, nv, dpc_u;
  FeTablesDev fe;
  const int32_t *cell_dofs_u, *cell_dofs_p; const double *cell_X;
  const double *cell_geo;   // [n_cells][10] or null (see poro_ctx::cell_geo)
  const uint8_t *dir_mask; const double *dir_val;
  poro_material mat;
  int interleaved_u;   // dof = node * dim + component everywhere (lets K-asm-u look CSR positions up per node pair)
  int mfg_sf;          // poro_ctx::mfg_sf: the sum-factorised general kernels may stand in for the table-driven one
  const double *cell_mod;   // [n_cells][2] = (lambda, G) per cell, or null: mat.lame_lambda / mat.shear_G (see poro_ctx::mod)
};
void asm_u_matrix(hipStream_t s, const AsmArgs &a, const int32_t *cells, int64_t n_cells, const int64_t *rp, const int32_t *col, double *val, double *lift);
void asm_u_element_matrix(hipStream_t s, const AsmArgs &a, int32_t cell, double *Ke);
void asm_u_rhs(hipStream_t s, const AsmArgs &a, const int32_t *cells, int64_t n_cells, const double *p, double *rhs);
// order / group_off: the boundary faces grouped by (colour of the cell, local face number), one launch per group (no atomics, fixed summation order)
void asm_u_neumann(hipStream_t s, const AsmArgs &a, const int32_t *order, const std::vector<int64_t> &group_off, const int32_t *bf_cell, const int32_t *bf_local, const int32_t *bf_id,
                   int n_neu, const int32_t *label, const int32_t *comp, const double *value, double *rhs);
// M, src == null: the Laplace matrix alone (K += K_c).  With cell_w ([n_cells][ncomp], K alone), ncomp == 1: K += cell_w[c] K_c, the per-cell coefficient of
// poro_ctx_set_cell_permeability; ncomp == dim: K += sum_q (sum_d cell_w[c][d] G_i[d] G_j[d]) JxW, the diagonal tensor of poro_ctx_set_cell_permeability_tensor
void asm_p_matrices(hipStream_t s, const AsmArgs &a, const int32_t *cells, int64_t n_cells, const int64_t *rp, const int32_t *col, double *M, double *K, double *src, const double *cell_w = nullptr,
                    int ncomp = 1);
void asm_proj_rhs(hipStream_t s, const AsmArgs &a, const int32_t *cells, int64_t n_cells, const double *u, int n_comp, const int32_t *comps /*host*/,
                  double *const *rhs /*host array of device ptrs*/);

// ---- kernels_gravity.hip: the gravity vectors (set-up only) ------------------------------------------
// out = the body-force vector of a uniform box, out[node * dim + d] = g_d sum_c rho_c int_c phi_node; rho_lattice: per cell in lattice order, or null: rho0
void box_body_u(hipStream_t s, int dim, int k_u, const BoxDev &box, const double *rho_lattice, double rho0, const double *g, double *out);
// out = -rho_f sum_c int_c (kappa_c g) . grad(phi_i) on a uniform box; kap_lattice: ncomp planes of per-cell weights in lattice order (ncomp = 1 | dim), or null: kap0
void box_gravity_p(hipStream_t s, int dim, const BoxDev &box, const double *kap_lattice, int ncomp, double kap0, double rho_f, const double *g, double *out);
// the same two on any mesh, added into `out` over the cells of one colour; cell_rho: [n_cells] or null: rho0; cell_w: [n_cells][ncomp] or null: kap0
void asm_u_body(hipStream_t s, const AsmArgs &a, const int32_t *cells, int64_t n_cells, const double *cell_rho, double rho0, const double *g, double *out);
void asm_p_gravity(hipStream_t s, const AsmArgs &a, const int32_t *cells, int64_t n_cells, const double *cell_w, int ncomp, double kap0, double rho_f, const double *g, double *out);

// ---- kernels_mfg.hip: matrix-free operator on general meshes (one wave per cell; coloured scatter, or one launch with an atomic scatter) ----------------
bool mfg_sf_tables_match(const poro_fe_tables &f, int dim, int k);
int mfg_apply(hipStream_t s, const AsmArgs &a, const int32_t *color_cells, const std::vector<int64_t> &color_off, int64_t n_u, const double *x, double *y, bool constrained, int mode,
              const int32_t *all_cells = nullptr /* non-null: ONE launch over this list of all cells with an atomic scatter (mode 0) */);
// ---- kernels_mf.hip -----------------------------------------------------------------------------
struct MfArgs { int dim, k_u; BoxDev box; const double *Ke; const uint8_t *mask; const double *diag_local; double lam, G; int mask_anywhere; const uint8_t *nodemask; const int32_t *dirichlet_dofs; int64_t n_dirichlet; };
void mf_apply(hipStream_t s, const MfArgs &a, const double *x, double *y, bool constrained, double *dot_partials = nullptr);
void mf_diag(hipStream_t s, const MfArgs &a, double *diag);
// y = (a M + kappa K) x for the Q1 pressure space of a uniform box (constant-coefficient 3^dim-point stencil)
void p_stencil_apply(hipStream_t s, int dim, const BoxDev &box, double a, double kappa, const double *x, double *y, const PcgScalars *gate = nullptr);      // gate: a no-op once gate->done (the pressure Newton loop's batch)
void p_residual_stencil(hipStream_t s, int dim, const BoxDev &box, double kappa, const double *t, const double *p, const double *src, double *R, const PcgScalars *gate = nullptr);
// the same with a per-cell coefficient: y = (a M + K_kappa) x, R = -((M t + K_kappa p) + q).  kap holds ncomp planes of n_cells weights in lattice cell order, ncomp = 1
// (one k / mu per cell) or dim (component d weights the derivatives along direction d, K_e = kx k(x)m(x)m + ky m(x)k(x)m + kz m(x)m(x)k)
void p_stencil_apply_var(hipStream_t s, int dim, const BoxDev &box, double a, const double *kap, int ncomp, const double *x, double *y);
void p_residual_stencil_var(hipStream_t s, int dim, const BoxDev &box, const double *kap, int ncomp, const double *t, const double *p, const double *src, double *R);

// polynomial-preconditioner step fused into the structured operator's stores: z_new = z_j + omega D^-1 (g - A z_j), D^-1 in dictionary form; z_new != z_j
struct KronCheb { const double *g = nullptr; double *znew = nullptr; double omega = 0; const uint8_t *cls = nullptr; const double *tab = nullptr;
                  // slab partitions: the raw partial product A z_j on the first / last node plane (the planes shared with the lower / upper neighbour) is written here as well
                  double *side_lo = nullptr, *side_hi = nullptr; };
// ---- kernels_kron.hip: sum-factorised (Kronecker) form of the same operator ---------------------------
bool kron_supported(int dim, int k_u);
void kron_prepare_device();   // per-device function attributes (dynamic LDS opt-in) of the structured kernels; call after hipSetDevice
BoxCoupling box_coupling(int dim, int k_u, const BoxDev &box);
void box_rhs_u(hipStream_t s, int dim, const BoxCoupling &B, double alpha, const double *p, const double *lift, const double *neu, const uint8_t *mask, double *rhs,
               const uint8_t *flags = nullptr /* box_rhs_u_flags of these lift and neu: the lines without nonzero entries are not read; null: all are */);
int64_t box_rhs_u_flag_count(int64_t n_u);
void box_rhs_u_flags(hipStream_t s, const double *lift, const double *neu, int64_t n_u, uint8_t *flags /*[box_rhs_u_flag_count(n_u)]*/);   // to be called again whenever lift or neu change
void box_asm_u_matrix(hipStream_t s, int dim, int k_u, const BoxDev &box, const double *Ke, const CsrDev &A, const uint8_t *mask, double *val);
void box_proj_rhs(hipStream_t s, int dim, const BoxCoupling &B, const double *u, int n_comp, const int32_t *tensor_components, double *const *rhs);
// all peers' windows in one launch: block q of the dense side is dense + q blk (to_block: peer `self` goes to dense_self instead - its own block of the receive buffer)
void fdm_window_batch(hipStream_t s, double *grid, double *dense, double *dense_self, int self, bool to_block, const FdmWindow *win, int n_peers, int n_planes_pad, int64_t C, int64_t grid_stride, int64_t blk);
void fdm_window(hipStream_t s, double *dst, const double *src, bool to_block, int n_planes, int n_planes_pad, int64_t C, int64_t ncols_valid, int64_t grid_stride, int64_t grid_col0, int64_t grid_plane0);
void fdm_transform(hipStream_t s, const double *T, int n_l, int64_t SI, int64_t n_outer, const double *in, double *out, const FdmScale *scale);
// layered per-cell coefficient: reciprocal pivots of the line systems (once per a), and the line solves themselves, between the x / y transforms (coef: perm_line.hpp)
// nw: the weighted mass lines of coef, one multiplier each (1: lam_x + lam_y on the one line; 2: the diagonal tensor in 3D, lam_x and lam_y on a line each)
void q1_line_factor(hipStream_t s, int dim, int nw, const FdmScalar &F, int nl, double a, const double *coef, double *inv);
void q1_line_solve(hipStream_t s, int dim, int nw, const FdmScalar &F, int nl, double a, bool fixed_lo, bool fixed_hi, const double *coef, const double *inv, const double *in, double *out);   // in != out, [plane of the slowest direction][column]
void fdm_apply(hipStream_t s, const FdmScalar &F, double a, const double k[3], const double *g, double *z, double *t1, double *t2);
// ---- kernels_fdmu.hip ---------------------------------------------------------------------------
void fdmu_upload_dir(FdmuDir &D, const LineTables &T, bool single, bool split);   // split: the even / odd form (T.parity required) unless a switch or `single` rules it out; D.split tells
// stage 2: the whole application (single rank); 0 / 1: the passes of the leading directions before / after the caller's distributed last direction
void fdmu_apply(hipStream_t s, const FdmU &F, const double *g, double *z, void *t1, void *t2, int stage);
void fdmu_window(hipStream_t s, double *dst, const double *src, bool to_block, int ncomp, int n_planes, int n_planes_pad, int64_t C, int64_t ncols_valid,
                 int64_t grid_stride, int64_t grid_planes, int64_t grid_col0, int64_t grid_plane0);
void fdmu_lines(hipStream_t s, const FdmU &F, const FdmuDir *last_dir, int64_t C, int64_t col0, int64_t ncol_valid, void *in, void *out);
// ---- kernels_fdmu_line.hip: the line solve that stands in for the last direction's transform pair when per-cell moduli are set (moduli_line.hpp) ----
// nl nodes per line, ncol columns per plane (x fastest, n0 of them per row); coef: [component][3][ku + 1][nl]; lam0 / lam1: the eigenvalues of the leading directions per
// component by position along x / y (lam1 null in 2D; not finite = removed mode); fixed[c][side]: component c is prescribed on that end face of the line direction
struct FdmuLineArgs { int nl, n0; int64_t ncol; const double *coef; const double *lam0[3], *lam1[3]; int fixed[3][2]; };
void fdmu_line_factor(hipStream_t s, int ku, int ncomp, const FdmuLineArgs &a, double *fac /*[ncomp][ku + 1][nl][ncol]: reciprocal pivots, multipliers*/);
void fdmu_line_solve(hipStream_t s, int ku, int ncomp, const FdmuLineArgs &a, const double *fac, double *v /*[ncomp][nl][ncol], in place*/);
// ---- kernels_fdmo.hip: octant form (see FdmOct) --------------------------------------------------
bool fdmo_usable(int dim, const int nn[3]);          // 3D, half lines of at most 128 entries (8 MFMA tiles)
void fdmo_init(FdmOct &O, const int nn[3], const double coef[3][3], hipStream_t s);   // sizes + buffers
// slab-partitioned form: nn = LOCAL nodes; layers[q] = node planes rank q holds minus one (its cell layers x degree); the last direction's matrices are uploaded for the GLOBAL line
void fdmo_init_slab(FdmOct &O, const int nn[3], const double coef[3][3], int rank, const std::vector<int> &node_layers, bool has_upper, hipStream_t s);
void fdmo_init_per_direction(FdmOct &O, const int nn[3], const double coef[3][3], const FdmFormDecision &D, hipStream_t s);   // per-direction form: sizes + buffers from the decision of fdm_form_decide
void fdmo_upload_dir(FdmOct &O, int comp, int dir, const LineTables &T);   // T.parity required (per-direction form: by its split directions only)
void fdmo_upload_dir_classes(FdmOct &O, int comp, int dir, const ClassSplitTables &T);   // octant form on one rank with O.class_split set (before the first upload): the class-split tables of the line, next to fdmo_upload_dir's
bool fdmo_class_split_runs(const FdmOct &O, int precision);   // whether fdmo_apply takes the class-split passes (k_fdmo_pass_vm) at this precision
void fdmo_finalize(FdmOct &O);   // after every (component, direction) has been uploaded: derived tables
void fdmo_apply(hipStream_t s, const FdmOct &O, const double *g_oct, double *z_oct, double *scratch_oct, const PcgScalars *gate = nullptr, hipEvent_t *ev /* optional: 3 start / stop pairs attached to the three pass dispatches */ = nullptr,
                double *gz_part /* optional: O.gz_part - pass 2 also leaves the O.gz_n partial sums of g . z there */ = nullptr,
                int precision /* PORO_FDM_FP32: the three passes on the fp32 MFMA with an fp32 intermediate array; g_oct, z_oct and g . z stay fp64 */ = PORO_FDM_FP64,
                const PcgStopTest &stop = PcgStopTest{} /* pass 1 runs the iteration's stopping test first; stop.sc == gate */);   // z = blockdiag(A_cc)^-1 g, all in octant form; gate: no-op once gate->done / finishing / stop
// the same transform kernel for the scalar Q1 systems of a 3D box (nodal layout, one block set, no octants): 3 launches instead of 6
bool fdmo_scalar_usable(int dim, const int nn[3]);
void fdmo_scalar_init(FdmOct &O, const int nn[3], hipStream_t s);
void fdmo_scalar_upload_dir(FdmOct &O, int dir, const LineTables &T);
int fdmo_scalar_apply(hipStream_t s, FdmOct &O, double a, double kappa, const double *g, double *z, const PcgScalars *gate = nullptr);   // both return the number of launches in the strip form (FdmOct::strip_limit)
int fdmo_scalar_apply_many(hipStream_t s, FdmOct &O, double a, double kappa, int nb, const double *const *g, double *const *z, const PcgScalars *gate = nullptr);   // up to 3 right-hand sides in one set of launches
// block partials of |y_e - b_e|^2 and |b_e|^2 for up to three (y, b) pairs: sets 2e and 2e + 1 of `partials`
// mask != null: rows with mask[i] != 0 count in neither norm (prescribed rows of a system solved on its free rows)
void la_residual_norms_many(hipStream_t s, int nb, const double *const *y, const double *const *b, int64_t n, double *partials, const uint8_t *mask = nullptr, const PcgScalars *gate = nullptr);
// slab partitions: nn = LOCAL vertices, the last direction's matrices are uploaded for the GLOBAL line; the three sweeps separately (all-to-alls in between, ctx_prec.hip)
void fdmo_scalar_init_slab(FdmOct &O, const int nn[3], int rank, const std::vector<int> &node_layers, hipStream_t s);
void fdmo_scalar_slab_pass(hipStream_t s, FdmOct &O, int pass, double a, double kappa, const double *in, double *out);
// planar (2D) form: quadrant layout with one plane and 2 components; four batched GEMM launches per application
bool fdmo_planar_usable(int dim, const int nn[3]);
void fdmo_init_planar(FdmOct &O, const int nn[3], const double coef[3][3], hipStream_t s, bool split = true /* false: different conditions at the two ends of some line - no parity split, full-length transforms */);
void fdmo_upload_dir_planar(FdmOct &O, int comp, int dir, const LineTables &T);   // T.parity required by the split form
void fdmo_apply_planar(hipStream_t s, const FdmOct &O, const double *g_q, double *z_q, const PcgScalars *gate = nullptr, const PcgStopTest &stop = PcgStopTest{} /* as fdmo_apply: in the first GEMM */);
void fdmo_from_nodal(hipStream_t s, const FdmOct &O, const double *v_nodal, double *q_oct);   // q = H v (node-interleaved vector -> octant form)
void fdmo_to_nodal(hipStream_t s, const FdmOct &O, const double *r_oct, double *v_nodal);     // v = H^-1-form of the backward transform: v_k = a + b, v_k' = a - b
// the vector kernels of pcg() with g / z in octant form (same device-side scalar protocol as their nodal counterparts in kernels_la.hip)
void fdmo_init_residual(hipStream_t s, const FdmOct &O, double *g_oct, const double *Ax, const double *b, const uint8_t *inert);
void fdmo_first_direction(hipStream_t s, const FdmOct &O, double *d, const double *g_oct, const double *z_oct, double *partials /*2 sets: gg, gz*/);
// red != null (partitioned runs): the all-reduced d.h (update_g: red[0]) / g.g and g.z (update_d: red[0], red[1]) instead of the block partials
void fdmo_update_g(hipStream_t s, const FdmOct &O, PcgScalars *sc, int parity, double *g_oct, const double *h, const uint8_t *inert, const double *partials_dh, double *partials_out /*gg*/, const double *red = nullptr);
void fdmo_update_d(hipStream_t s, const FdmOct &O, PcgScalars *sc, int parity, int it, double *x, double *d, const double *z_oct, const double *partials_in /*2 sets*/, const double *red = nullptr,
                   bool gz_from_pass = false /* g . z from O.gz_part (left by fdmo_apply) instead of the second set of partials_in */,
                   bool stream_x = false /* three components: non-temporal accesses to x (the caller keeps h in z's allocation, see pcg) */,
                   bool decided = false /* the preconditioner call in front ran the stopping test (PcgStopTest): take sc->stop instead of testing */,
                   bool gg_stored = false /* with `decided`: take g . g from PcgScalars::gg, where that test left the sum of the first set of partials_in, instead of adding them up again */);
void fdmo_dot_owned(hipStream_t s, const FdmOct &O, const double *a_oct, const double *b_oct, double *partials, const PcgScalars *gate);   // block partials of a.b over the planes this rank owns
// slab form: the pieces of one application around the two all-to-alls (ctx_prec.hip drives them)
void fdmo_slab_pass(hipStream_t s, const FdmOct &O, int pass /*1, 2, 3*/, const double *in, double *out, const PcgScalars *gate, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
// pass 1: quadrant layout -> slab.buf (send half; own share -> receive half); pass 2: gathered planes in slab.buf -> slab.tz; pass 3: scattered planes in slab.buf -> quadrant layout
void fdmo_slab_scatter_pack(hipStream_t s, const FdmOct &O, const PcgScalars *gate);                            // slab.tz -> slab.buf (inverse butterfly; every rank's planes incl. the shared ones)
// dot_partials (optional, kMaxPartials slots, zeroed by the caller once): per-workgroup partial sums of x.y, fused into the apply
int kron_apply(hipStream_t s, const MfArgs &a, const double *x, double *y, bool constrained, int n_cus, double *dot_partials = nullptr, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr,
               const PcgScalars *pcg = nullptr /* launch becomes a no-op once pcg->done / finishing is set */,
               const KronCheb *cheb = nullptr /* 3D only: store the Chebyshev update instead of the product (y is not written) */);   // returns the workgroup count (= partial slots used)
void kron_fix_constrained(hipStream_t s, const MfArgs &a, const double *x, double *y, double *dot_partials, int slot_base);
// ---- kernels_kron_lm.hip: the same operator on a 3D box with lambda, G layered along z (poro_ctx_set_moduli_operator) ----
void kron_lm_prepare_device();   // as kron_prepare_device
// planes: device copy of moduli_plane_table (moduli_planes.hpp); arguments and return value as kron_apply
int kron_lm_apply(hipStream_t s, const MfArgs &a, const double *planes, const double *x, double *y, bool constrained, int n_cus, double *dot_partials = nullptr, hipEvent_t ev0 = nullptr,
                  hipEvent_t ev1 = nullptr, const PcgScalars *pcg = nullptr);
// ---- kernels_hyb.hip: the pieces of the hybrid operator form between the fine-cell launches and the box product ------------------
void hyb_gather(hipStream_t s, int dim, int64_t n_box_nodes, const int64_t *inj, const double *x, double *x_box);   // x_box[b] = x[inj[b]], node-wise
// y[inj[b]] += y_box[b] - sum over the refined box cells around b of (Ke x_box)'s row of b; `box` = mf_args of the box context (geometry, nodemask: Dirichlet columns zeroed
// when constrained), Ke_t = its element matrix transposed; the pointers of HybridPlan
struct HybCombine { int64_t n_box_nodes, n_removed, n_chunks; const int64_t *inj; const uint8_t *touched; const int32_t *removed_cells, *slot, *chunk_cls; const int64_t *nodes;
                    const double *x_box, *y_box; double *V; };
void hyb_combine(hipStream_t s, const MfArgs &box, const double *Ke_t, bool constrained, const HybCombine &h, double *y);

}  // namespace poro
