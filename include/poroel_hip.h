/*
 * poroel_hip.h — C-ABI of the MI355X-native fixed-stress Biot hot path.
 *
 * This is the drop-in boundary for the per-timestep "assemble + Krylov solve"
 * path of ishovkun/poroelasticity-dealii.  The reference has no FFI; the path
 * sits behind public member functions of three class templates that are only
 * called from PoroElasticProblem<dim>::run() (lib/include/PoroelasticityFSS.h:294-415).
 * Every entry point below names the reference member (file:line) it replaces.
 * Signatures use plain pointers and sizes only (no C++/torch types); the
 * library owns all device memory behind the opaque handle, the caller owns the
 * host arrays it passes in.  Entry points that hand something back to the host (a norm, a
 * poro_solve_info, a vector, a matrix) return when the device has produced it; entry points that
 * only transform device-resident state (assembly, vector updates, the `distribute` at the end of a
 * solve) are ordered on the context's stream and may return before the device has finished - exactly
 * what lets the fixed-stress loop run without idling the GPU between calls.  poro_ctx_synchronize()
 * waits for everything enqueued so far; errors of asynchronous work surface at the next
 * synchronising call.
 *
 * Conventions fixed by this ABI (the reference leaves them to deal.II):
 *   - local scalar nodes of a cell are lexicographic on the (k+1)^dim tensor
 *     grid, x fastest; local vector dof i = scalar_node*dim + component
 *     (FESystem::system_to_component_index, PoroElasticDisplacementSolver.h:218);
 *   - cell vertices are lexicographic (v = ix + 2*iy + 4*iz), as deal.II;
 *   - faces: f = 2*normal_direction + (0 low side | 1 high side), as deal.II
 *     GeometryInfo; hyper_rectangle(colorize) boundary ids equal f
 *     (PoroelasticityFSS.h:430-432, input.data:8-11);
 *   - quadrature points are tensorised Gauss-Legendre on [0,1], x fastest
 *     (QGauss<dim>, PoroElasticDisplacementSolver.h:159);
 *   - all floating point data is IEEE double; dof/cell indices are int32,
 *     CSR row pointers int64.
 *
 * Return codes: 0 ok; >0 a Krylov solve hit its iteration cap (the analogue of
 * deal.II SolverControl::NoConvergence, info is filled); <0 invalid argument,
 * HIP or RCCL failure (message via poro_last_error()).
 */
#ifndef POROEL_HIP_H
#define POROEL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PORO_ABI_VERSION 4   /* 4: poro_desc.tensor (tensor-product grids keep the fast-diagonalisation preconditioners), poro_desc.coarse + PORO_PREC_TWO_LEVEL;  2: poro_solver_opts.omega, PORO_PREC_SSOR / FDM / ILU0, PORO_VEC_STRESS0; 3: poro_solver_opts.stop_rule / poly_degree, poro_constraints, PORO_PREC_FDM and PORO_PREC_CHEBYSHEV for the displacement system, general form of poro_partition, prescribed pressures */

/* Reference-cell tables: exactly the numbers the reference pulls out of
 * FEValues / FEFaceValues (PoroElasticDisplacementSolver.h:162-173,
 * StrainProjector.h:127-134, MatrixCreator calls PoroElasticPressureSolver.h:96-101).
 * "q1" is the Q1 Lagrange basis on the cell vertices: it is both MappingQ1 and
 * the pressure element FE_Q(1) (PoroElasticPressureSolver.h:20,57). */
typedef struct poro_fe_tables {
  int32_t nq_u;  /* (k_u+1)^dim  volume points, QGauss(fe.degree+1) of u      */
  int32_t nq_p;  /* 2^dim        volume points, QGauss(2) of p                */
  int32_t nq_f;  /* (k_u+1)^(dim-1) face points                               */
  int32_t ns_u;  /* scalar nodes per cell of u: (k_u+1)^dim                   */
  int32_t ns_p;  /* = number of vertices 2^dim                                */
  const double *w_qu;      /* [nq_u]                                          */
  const double *w_qp;      /* [nq_p]                                          */
  const double *w_qf;      /* [nq_f]                                          */
  const double *u_qu;      /* [nq_u][ns_u]        phi^u_s(xi_q)               */
  const double *du_qu;     /* [nq_u][ns_u][dim]   d phi^u_s / d xi_d          */
  const double *du_qp;     /* [nq_p][ns_u][dim]                               */
  const double *q1_qu;     /* [nq_u][ns_p]                                    */
  const double *dq1_qu;    /* [nq_u][ns_p][dim]                               */
  const double *q1_qp;     /* [nq_p][ns_p]                                    */
  const double *dq1_qp;    /* [nq_p][ns_p][dim]                               */
  const double *u_qf;      /* [2*dim][nq_f][ns_u] u shape values on face f    */
  const double *dq1_qf;    /* [2*dim][nq_f][ns_p][dim]                        */
} poro_fe_tables;

/* Constant coefficients, = InputDataPoroel after compute_derived_parameters
 * (InputDataPoroel.h:213-222; units :162,168). */
typedef struct poro_material {
  double lame_lambda;   /* data.lame_constant  */
  double shear_G;       /* data.shear_modulus  */
  double biot_alpha;    /* data.biot_coef      */
  double bulk_K;        /* data.bulk_modulus (drained)  */
  double biot_M;        /* data.m_modulus      */
  double k_over_mu;     /* data.perm/data.visc */
  double r_well;        /* data.r_well         */
  double flow_rate;     /* data.flow_rate      */
} poro_material;

/* Optional: the mesh is a uniform box n[0] x n[1] (x n[2]) with lexicographic
 * node numbering and dof = node*dim + comp (u), dof = vertex (p).  Enables the
 * matrix-free operator.  hyper_rectangle + refine_global meshes
 * (PoroelasticityFSS.h:418-435) are of this kind. */
typedef struct poro_structured {
  int32_t enabled;
  int32_t n[3];
  double  origin[3];
  double  h[3];
} poro_structured;

/* Optional: the mesh is a TENSOR-PRODUCT grid - topology and numbering as for a poro_structured box with n[] cells per direction, vertex planes of direction d at
 * grid[d][0 .. n[d]] (ascending, any spacing), e.g. a graded hyper_rectangle.  The cells are not congruent, so the structured operator kernels do not
 * apply (the general matrix-free operator runs), but the fast-diagonalisation preconditioners stay exact: their 1D FE matrices are assembled on the
 * given 1D grids (PORO_PREC_FDM for all three systems; one rank).  Ignored when box.enabled. */
typedef struct poro_tensor_grid {
  int32_t enabled;
  int32_t n[3];
  const double *grid[3];   /* [n[d] + 1] each */
} poro_tensor_grid;

/* Optional coarse space for the two-level preconditioner of the displacement system (PORO_PREC_TWO_LEVEL): the mesh is a refinement of a uniform box - a locally
 * refined hyper_rectangle (refine_mesh, PoroelasticityFSS.h:447-498) - whose own description is `box_problem` (same material and boundary conditions, box tag
 * set; it must stay alive until poro_ctx_create has returned), and every displacement NODE i of this mesh (= dof / dim: the numbering must be node-interleaved)
 * interpolates the box's FE functions: v_h(node i) = sum_k weight[k] * v_H(node[k]), k in ptr[i] .. ptr[i+1].
 * One rank, or a GENERAL partition (poro_partition.n_neighbours > 0; refused on slab partitions).  On a general partition:
 *   - box_problem is the whole, unpartitioned box, the same on every rank (the coarse solve runs replicated on each rank);
 *   - ptr / node / weight hold one row per LOCAL node (owned, shared and ghost alike), ptr_p / node_p / weight_p one per local pressure dof; the rows of a dof that
 *     several ranks hold must be identical (same entries, same order) on all of them;
 *   - the displacement numbering must keep whole nodes: node-interleaved incl. the ghost dofs, n_dofs_u and n_owned_u multiples of dim (owned nodes first);
 *   - every rank passes a coarse space or none.  The library cannot check this at poro_ctx_create (no communicator exists yet): a rank without one would not join the
 *     all-reduce that every application of PORO_PREC_TWO_LEVEL performs (the owned rows' restriction P^T g, 8 * dim * box nodes bytes; 8 * box vertices for the scalar
 *     systems).  The host provider's pieces (poro_host_partition_ex with the coarse flag) satisfy all of this. */
struct poro_desc;
typedef struct poro_coarse_space {
  int32_t enabled;
  const struct poro_desc *box_problem;
  const int64_t *ptr;       /* [n_dofs_u / dim + 1] */
  const int32_t *node;      /* [ptr[last]] coarse node numbers */
  const double  *weight;
  /* optional: the same for the pressure space (dof i = sum weight_p[k] * box pressure dof node_p[k]): PORO_PREC_TWO_LEVEL for the pressure and projection solves */
  const int64_t *ptr_p;     /* [n_dofs_p + 1] or NULL */
  const int32_t *node_p;
  const double  *weight_p;
} poro_coarse_space;

/* Partition over ranks.  Slab form for a structured box:  The local mesh is
 * the rank's slab as a standalone box; node planes at the low / high end in the
 * slowest direction are shared with the neighbour rank when has_lower/has_upper. */
typedef struct poro_partition {
  int32_t rank, n_ranks;
  int32_t has_lower, has_upper;
  int64_t plane_u;   /* u dofs on one interface plane  */
  int64_t plane_p;   /* p dofs on one interface plane  */
  /* General partition (any mesh; SURVEY 8e: contiguous cell ranges + an indexed interface list), used when n_neighbours > 0 (then has_lower /
   * has_upper / plane_* are ignored).  The local mesh is the rank's cells as a standalone mesh; a dof touched by cells of several ranks is
   * local to each of them.  Local dofs [0, n_owned) are the ones this rank owns (every shared dof has exactly one owner; dots run over owned
   * dofs), the others follow.  shared_dof_*[shared_ptr_*[k] .. shared_ptr_*[k+1]) are the local dofs shared with rank neighbour_rank[k], listed
   * in the SAME order on both sides (e.g. ascending global index); a dof shared by three ranks appears in two lists on each of them.  Partial
   * sums are exchanged pairwise and added in ascending rank order, so every rank holding a dof computes bitwise the same value. */
  int32_t n_neighbours;
  const int32_t *neighbour_rank;   /* [n_neighbours], ascending, without `rank` */
  const int64_t *shared_ptr_u;     /* [n_neighbours + 1] */
  const int32_t *shared_dof_u;
  const int64_t *shared_ptr_p;     /* [n_neighbours + 1] */
  const int32_t *shared_dof_p;
  int64_t n_owned_u, n_owned_p;
} poro_partition;

/* Closed affine constraints beyond the Dirichlet list: the hanging nodes of a locally refined mesh (DoFTools::make_hanging_node_constraints,
 * PoroElasticDisplacementSolver.h:112-113, PoroElasticPressureSolver.h:72-75; refine_mesh, PoroelasticityFSS.h:447-498).
 *   x[dof[i]] = sum_{k in ptr[i]..ptr[i+1]} weight[k] * x[master[k]] + inhomogeneity[i]
 * (Partitioned runs, general form of poro_partition: every rank passes the entries whose constrained dof is local to it, and every master of such an entry must be
 * local too - where none of the rank's cells touches a master it becomes a local dof of no local cell, listed in the interface lists of all ranks that hold it.)
 * exactly what ConstraintMatrix holds after close(): masters are unconstrained dofs, a constrained dof appears once and is not in the
 * Dirichlet list.  The library condenses at operator level (C^T A C on the free dofs, C^T b), which gives the same solution as
 * ConstraintMatrix::condense / distribute_local_to_global (:153, :168, PoroElasticDisplacementSolver.h:280-286), and distributes after each solve (:180, :306). */
typedef struct poro_constraints {
  int64_t n;
  const int32_t *dof;            /* [n]      */
  const int64_t *ptr;            /* [n+1]    */
  const int32_t *master;         /* [ptr[n]] */
  const double  *weight;         /* [ptr[n]] */
  const double  *inhomogeneity;  /* [n]      */
} poro_constraints;

typedef struct poro_desc {
  int32_t abi_version;
  int32_t dim;        /* 2 | 3 */
  int32_t degree_u;   /* 1 | 2  (the reference hard-wires 2, PoroElasticDisplacementSolver.h:67) */
  int32_t degree_p;   /* 1 */
  int64_t n_cells, n_vertices, n_dofs_u, n_dofs_p;
  const double  *vertex_coords;  /* [n_vertices][dim]                       */
  const int32_t *cell_vertices;  /* [n_cells][2^dim]                        */
  const int32_t *cell_dofs_u;    /* [n_cells][dim*ns_u]  cell->get_dof_indices (:279) */
  const int32_t *cell_dofs_p;    /* [n_cells][ns_p]      (StrainProjector.h:191)      */
  poro_fe_tables fe;
  /* boundary faces, for the Neumann term (:249-277) */
  int64_t n_bfaces;
  const int32_t *bface_cell, *bface_local, *bface_id;
  /* closed Dirichlet constraint list = `constraints` after :117-136 */
  int64_t n_dirichlet;
  const int32_t *dirichlet_dof;
  const double  *dirichlet_value;
  /* Neumann conditions (BoundaryConditions.h:45-62) */
  int32_t n_neumann;
  const int32_t *neumann_label, *neumann_component;
  const double  *neumann_value;
  poro_material   mat;
  poro_structured box;
  poro_partition  part;
  poro_constraints cons_u;   /* displacement space (n = 0: none) */
  poro_constraints cons_p;   /* pressure space; also used by the strain projection (StrainProjector.h:191-194) */
  /* EXTENSION (not in the reference, whose pressure space has "no dirichlet pressure BC's", PoroElasticPressureSolver.h:69-70): prescribed pressures,
   * e.g. a drained boundary p = 0.  Needed to validate the corrected-physics switches on Terzaghi's consolidation problem.  The rows are
   * taken out of the pressure Newton system (residual 0, update 0); poro_pres_apply_boundary_values writes the values into PORO_VEC_P.
   * One rank.  Preconditioners of poro_pres_solve: PORO_PREC_JACOBI / NONE for any set.
   * Where the set is exactly a union of whole faces of a uniform box (box.enabled) or tensor-product grid (tensor) - the values may differ from node to node -
   * also PORO_PREC_FDM: the free block of a M + kappa K is then a Kronecker sum of the 1D matrices without those end nodes and has its own exact fast
   * diagonalisation (direct solve on matrix-free boxes, info.iterations = 0; preconditioner of CG on tensor grids and CSR contexts); the update is exactly 0
   * on the prescribed rows (that path first zeroes PORO_VEC_RESIDUAL_P and PORO_VEC_DP there: the rows are not part of the system, whatever a caller stored in them).
   * poro_supports_preconditioner(ctx, 1, PORO_PREC_FDM) tells.  The projection (which_system = 2) is not affected by the list.
   * Together with hanging pressure nodes (cons_p; a drained face on a locally refined mesh) the two lists are analysed at set-up.  A hanging dof may have prescribed
   * masters (the normal case; its row then reads their values).  A dof may be in BOTH lists only if all its masters are prescribed and its value is
   * sum w * value(master) + inhomogeneity, to 1e-12 of the largest prescribed magnitude (1e-12 absolute if that is 0); any other overlap is refused with the dof
   * named.  The Newton system is C^T J C without the prescribed rows: residual condensed first, then zeroed on the prescribed rows; the update is 0 on the prescribed
   * rows and distributed homogeneously, so a dof in both lists gets 0.  PORO_PREC_FDM is not available there (hanging nodes).  PORO_PREC_TWO_LEVEL, with or
   * without hanging nodes: where poro_desc.coarse.box_problem carries a prescribed set of its own that covers whole faces, and every dof of this mesh whose
   * interpolation row is a single entry of weight 1 on a prescribed coarse dof is prescribed here too; the coarse solve is then the box's matrix without those
   * faces, z = omega D^-1 g + P (J_H)_ff^-1 P^T g.  poro_supports_preconditioner(ctx, 1, PORO_PREC_TWO_LEVEL) tells. */
  int64_t n_dirichlet_p;
  const int32_t *dirichlet_dof_p;
  const double  *dirichlet_value_p;
  poro_tensor_grid tensor;
  poro_coarse_space coarse;
} poro_desc;

/* Krylov controls.  Reference values: displacement abs 1e-12, 1000 its
 * (PoroElasticDisplacementSolver.h:298-299); pressure / projection
 * rel 1e-8*||rhs||, 1000 its (PoroElasticPressureSolver.h:175, StrainProjector.h:209).
 * Stopping test is on the recursively updated residual: ||g||_2 <= max(abs_tol, rel_tol*||b||_2) (PORO_STOP_RHS, what the
 * reference's three SolverControl objects express), or ||g||_2 <= max(abs_tol, rel_tol*||g_0||_2) with g_0 the residual of the
 * warm start (PORO_STOP_REDUCTION = deal.II ReductionControl): a transient whose right-hand side barely changes from step to step
 * still solves every step to the same relative accuracy instead of accepting the warm start. */
typedef struct poro_solver_opts {
  double  abs_tol;
  double  rel_tol;
  int32_t max_iter;
  int32_t preconditioner;  /* PORO_PREC_* */
  double  omega;           /* relaxation of PORO_PREC_SSOR: 1.2 displacement (:303), 1.0 pressure / projection (:178, StrainProjector.h:212) */
  int32_t stop_rule;       /* PORO_STOP_* */
  int32_t poly_degree;     /* PORO_PREC_CHEBYSHEV: operator applications per preconditioner call (<= 0: 6; odd values are rounded up); `omega` then holds the ratio lambda_max / a of
                              the interval [a, lambda_max] the polynomial is built for (<= 0: a mesh-size based default) */
} poro_solver_opts;
enum { PORO_STOP_RHS = 0, PORO_STOP_REDUCTION = 1 };

/* PORO_PREC_SSOR = PreconditionSSOR in the matrix's natural row order (level-scheduled sweeps; assembled-CSR operators only):
 * reproduces the reference's Krylov iterates, at many small launches per application - a fidelity mode, not the fast path.
 * PORO_PREC_FDM = fast diagonalisation: on a uniform box (poro_desc.box.enabled; slab-partitioned runs included) the pressure Jacobian and the projection
 * mass matrix are sums of Kronecker products of 1D matrices and are inverted exactly by 2*dim batched dense transforms (fp64 MFMA);
 * CG keeps the reference's stopping rule and needs 1-2 iterations.  poro_supports_preconditioner() tells whether a context can.
 * For the displacement system PORO_PREC_FDM is the BLOCK fast diagonalisation: the diagonal blocks A_cc of the elasticity operator (one per
 * displacement component) are Kronecker sums of 1D FE_Q(k) matrices whenever every Dirichlet condition covers whole faces, and are inverted
 * exactly the same way (per-component 1D eigenvectors, fp64 MFMA transforms); CG on a 10 M-dof box then takes ~20 iterations instead of ~250.
 * PORO_PREC_ILU0 = incomplete LU on the pattern of the assembled CSR matrix (factorised once per matrix ON THE DEVICE, level-scheduled in the natural
 * row order like the triangular solves, so the factors equal those of a sequential IKJ sweep; one rank, moderate sizes).
 * PORO_PREC_CHEBYSHEV (displacement system) = Chebyshev polynomial in D^-1 A of degree poly_degree around the Jacobi preconditioner: the CG iteration
 * count drops by about the degree + 1 while the operator applications of the polynomial need no dot products and, on 3D boxes, no vector kernels either
 * (the update z_{j+1} = z_j + D^-1 (g - A z_j) / r_j - roots r_j of the shifted Chebyshev polynomial - is applied inside the structured operator kernel where the product leaves the registers): fewer bytes and far fewer reductions per
 * operator application than Jacobi-CG.  lambda_max(D^-1 A) comes from the Lanczos tridiagonal of 25 Jacobi-CG steps when the matrix is (re)built (+5 %,
 * capped on uniform boxes by the rigorous element bound lambda_max(diag(K_e)^-1 K_e)).
 * PORO_PREC_TWO_LEVEL (displacement system; meshes with poro_desc.coarse, i.e. locally refined boxes with their hanging-node constraints) = additive two-level
 * preconditioner z = omega D^-1 g + P B_H^-1 P^T g: Jacobi on the refined mesh plus the BLOCK fast diagonalisation of the underlying uniform box as coarse solve (P = the
 * FE interpolation of poro_coarse_space).  The CG iteration count stays bounded under uniform refinement of the whole configuration.  With poro_coarse_space.ptr_p ...
 * also for poro_pres_solve (a M + kappa K: Jacobi + the box's exact scalar fast diagonalisation through the vertex interpolation; hanging nodes allowed, prescribed
 * pressures where the coarse box carries them as whole faces, see poro_desc.dirichlet_dof_p) and poro_proj_solve (accepted; Jacobi alone is already mesh-independent on the mass matrix and needs fewer iterations). */
enum { PORO_PREC_NONE = 0, PORO_PREC_JACOBI = 1, PORO_PREC_SSOR = 2, PORO_PREC_FDM = 3, PORO_PREC_ILU0 = 4, PORO_PREC_CHEBYSHEV = 5, PORO_PREC_TWO_LEVEL = 6 };
enum { PORO_OP_CSR = 0, PORO_OP_MATRIX_FREE = 1 };
enum { PORO_MAT_A_U = 0, PORO_MAT_MASS_P = 1, PORO_MAT_LAPLACE_P = 2, PORO_MAT_JACOBIAN_P = 3 };
enum { PORO_VEC_U = 0, PORO_VEC_RHS_U = 1, PORO_VEC_P = 2, PORO_VEC_P_OLD = 3, PORO_VEC_DP = 4,
       PORO_VEC_RESIDUAL_P = 5, PORO_VEC_EPSV = 6, PORO_VEC_EPSV0 = 7, PORO_VEC_SOURCE_P = 8,
       PORO_VEC_STRAIN0 = 16 /* + packed symmetric entry (TensorIndexer.h:24-31) */,
       PORO_VEC_PROJ_RHS0 = 32 /* + entry */, PORO_VEC_DIAG_U = 48,
       PORO_VEC_STRESS0 = 64 /* + packed symmetric entry: nodal effective stress (PoroelasticityFSS.h:189-224) */ };

typedef struct poro_solve_info {
  int32_t iterations;
  int32_t converged;
  double  initial_residual;
  double  final_residual;
  double  seconds;       /* wall time of the solve on device */
  int64_t operator_applications;   /* of the Krylov solves: iterations + 1 (the initial residual and one per iteration); iterations + 2 where a partitioned run takes the
                                      single-reduction recurrence (it applies the operator to P^-1 g before it knows that g has converged; Jacobi, no preconditioner, block
                                      FDM outside the slab form, two-level); (poly_degree + 1) * (iterations + 1) with PORO_PREC_CHEBYSHEV on either recurrence - the USEFUL
                                      applications: the single-reduction recurrence launches one polynomial and one operator application more, for the last z.  The SSOR /
                                      ILU(0) fidelity modes count what they applied; a direct fast-diagonalisation solve reports 1 (the check of its residual) */
} poro_solve_info;

typedef struct poro_ctx poro_ctx;

const char *poro_last_error(void);
int  poro_abi_version(void);

/* setup_dofs of the three solvers (PoroElasticDisplacementSolver.h:106-153,
 * PoroElasticPressureSolver.h:68-111, StrainProjector.h:82-98): builds sparsity,
 * mass / Laplace matrices, constraint tables, device vectors.  operator_mode
 * selects assembled CSR or the matrix-free A_u (needs desc->box.enabled). */
int  poro_ctx_create(const poro_desc *desc, int device, int operator_mode, poro_ctx **out);
void poro_ctx_destroy(poro_ctx *ctx);
/* wait until the device has finished everything the context has enqueued (see the note on synchronisation at the top) */
int  poro_ctx_synchronize(poro_ctx *ctx);

/* Scatter mode of the matrix-free operator on GENERAL meshes (no box tag): how the cell loop adds its contributions into y = A_u x.
 *   PORO_SCATTER_COLOURED (default): one launch per colour class (2^dim), plain read-modify-write, bitwise reproducible.
 *   PORO_SCATTER_ATOMIC:             ONE launch over all cells, fp64 atomic adds; the results differ in the last bits from run to run.
 * May be changed between any two calls; governs every application of the operator (Krylov operator, Chebyshev polynomial, two-level fine-level products, partitions,
 * condensation, poro_apply_operator / poro_bench_operator).  The set-up quantities (diagonal, lifting vector, the product with the constraints' inhomogeneities in the
 * condensed right-hand side, self-checks) stay coloured in both modes: PORO_VEC_DIAG_U and PORO_VEC_RHS_U do not depend on the mode, bit for bit.  The cell list of
 * the single launch (4 bytes per cell) is built on the host from the cell vertices when a context enters the atomic mode for the first time (a stream synchronise, a
 * device-to-host copy of the vertices and a sort: call it outside timed regions; under the environment variable below the first operator application pays for it).  On a box-tagged
 * context the call succeeds and changes nothing (the structured kernels have no scatter).  An unknown mode returns < 0.  The environment variable
 * PORO_MFG_SCATTER=atomic|coloured (diagnostic) is read once, at context creation, as the initial mode. */
enum { PORO_SCATTER_COLOURED = 0, PORO_SCATTER_ATOMIC = 1 };
int  poro_ctx_set_scatter_mode(poro_ctx *ctx, int32_t mode);
int  poro_ctx_get_scatter_mode(poro_ctx *ctx, int32_t *mode);

/* Operator form of the matrix-free operator on REFINED BOXES (a uniform box with some cells split once, poro_desc.coarse = the uniform box; no box tag).
 *   PORO_OPFORM_GENERAL (default): the general cell kernels over every cell.
 *   PORO_OPFORM_HYBRID:            A x = S (A_box x_box - sum_{refined box cells c} K_c x_box) + sum_{fine cells f} K_f x,  x_box = S^T x, S = the injection box node ->
 *                                  mesh node: the box's structured kernel over the whole box, the element matrix on the refined box cells (subtracted, owner computes), the
 *                                  general cell kernels over the children only.  The results differ from the general form's by rounding (a few ulps of the sum of the
 *                                  contributions); in PORO_SCATTER_COLOURED they are bitwise reproducible from call to call.
 * May be changed between any two calls; governs the same applications as the scatter mode (Krylov operator, Chebyshev polynomial, two-level fine-level products,
 * condensation, poro_apply_operator / poro_bench_operator) and composes with it: the fine-cell launches run in the context's scatter mode.  The set-up quantities
 * (diagonal, lifting vector, the product with the constraints' inhomogeneities, self-checks) keep the general coloured form: PORO_VEC_DIAG_U and PORO_VEC_RHS_U do
 * not depend on the form, bit for bit.
 * The library derives everything itself from what the context holds, at the FIRST enable: the injection from the interpolation rows (box node b <-> the mesh node whose
 * row is the single entry (b, 1.0)), the unrefined cells (dof list = the injected dof list of a box cell), the refined box cells (matched by none) and the fine cells (the
 * rest: 2^dim per refined box cell), then compares one hybrid product with the general one (skipped under PORO_DIAG_SKIP_SELFCHECK=1).  That first enable costs
 * device-to-host copies of the cell lists and vertices, host work, uploads, two box-sized device vectors and a stream synchronise: call it outside timed regions.
 * Returns < 0 with a message, the form staying as it was, on: no coarse space; a partitioned context; a context not created with PORO_OP_MATRIX_FREE; a dimension /
 * degree without structured kernel; a box node without injected image (an auxiliary box); unmatched cells; vertices of a matched cell more than 1e-12 of the box
 * extent off the box cell's (a mapped mesh); a Dirichlet mask that differs from the box's at the injected dofs; different material constants; a failed self-check;
 * an unknown form.  On a box-tagged context the call succeeds and changes nothing.  The form is never chosen automatically.
 * The getter also reports the cells the general kernels run over per application (all cells in the general form, the fine cells in the hybrid one, 0 on a box-tagged
 * context) and the refined box cells whose element products are subtracted (0 in the general form); either pointer may be NULL. */
enum { PORO_OPFORM_GENERAL = 0, PORO_OPFORM_HYBRID = 1 };
int  poro_ctx_set_operator_form(poro_ctx *ctx, int32_t form);
int  poro_ctx_get_operator_form(poro_ctx *ctx, int32_t *form, int64_t *general_cells /* cells the general kernel runs over per application */, int64_t *removed_box_cells);

/* Transform precision of PORO_PREC_FDM for the DISPLACEMENT system, where it runs in the single-rank 3D octant form (one rank, 3D, every Dirichlet condition on a pair of
 * opposite faces, half lines of at most 128 nodes).
 *   PORO_FDM_FP64 (default): the three transform passes on the fp64 matrix instruction.
 *   PORO_FDM_FP32:           the same passes on the fp32 matrix instruction, fp32 transform matrices and an fp32 intermediate array; the residual, the preconditioned
 *                            residual, g . z, the operator, the iterate and the stopping test stay fp64 (a lower-precision preconditioner inside an fp64 CG).
 * Governs poro_disp_solve and poro_apply_preconditioner_u (its `reps` timing included).  Everything else stays fp64 in both modes: the scalar Q1 systems (there the fast
 * diagonalisation is an exact direct solve), the planar 2D form, the slab / quadrant form of partitioned runs, the nodal fallback kernels and the coarse box of
 * PORO_PREC_TWO_LEVEL.  On a context that does not run the octant form the setter succeeds, `effective` reports PORO_FDM_FP64 and nothing changes bit for bit.
 * May be changed between any two calls, at no cost: the fp32 copies of the transform matrices are uploaded next to the fp64 ones when the block FDM is built (the first
 * solve with PORO_PREC_FDM, or the getter below).  `effective` is final only once the block FDM has been built (the build checks the eigenvectors' mirror symmetry numerically),
 * so poro_ctx_get_fdm_precision BUILDS it when fp32 is requested on a single-rank 3D context that can use PORO_PREC_FDM: host eigenproblems, uploads and a stream
 * synchronise - call it outside timed regions.  With PORO_FDM_FP64 requested the getter builds nothing.
 * Range: the fp32 mode needs |g| and |g| / den (den = the eigenvalue sums of the blocks, of the size of the moduli / h) to be fp32-normal, roughly 1e-38 .. 3e38; with GPa
 * moduli and the reference's tolerances the residual at the end of a solve sits near 1e-25.  Nothing checks this at run time.
 * The mode is never chosen automatically.  An unknown value returns < 0 with a message.  The environment variable PORO_FDMO_PRECISION=fp32|fp64 is read once, at context
 * creation, as the initial mode (so that unchanged drivers can run it); PORO_FDMU_SINGLE keeps its own meaning (fp32 nodal transforms, octant form off). */
enum { PORO_FDM_FP64 = 0, PORO_FDM_FP32 = 1 };
int  poro_ctx_set_fdm_precision(poro_ctx *ctx, int32_t precision);
int  poro_ctx_get_fdm_precision(poro_ctx *ctx, int32_t *requested, int32_t *effective);

/* multi-GPU wiring.  id is the 128-byte ncclUniqueId from rank 0. */
int  poro_comm_unique_id(void *id128);
int  poro_ctx_comm_init_rccl(poro_ctx *ctx, const void *id128);
/* host-staged exchange through caller callbacks (tests: 2 ranks on one GPU, gloo). */
typedef void (*poro_allreduce_fn)(double *buf, int32_t n, void *user);
typedef void (*poro_sendrecv_fn)(const double *send, double *recv, int64_t n, int32_t peer, void *user);
int  poro_ctx_comm_init_callbacks(poro_ctx *ctx, poro_allreduce_fn ar, poro_sendrecv_fn sr, void *user);

/* vectors live on the device between calls; these move them across the boundary */
int  poro_vec_set(poro_ctx *ctx, int which, const double *host, int64_t n);
int  poro_vec_get(poro_ctx *ctx, int which, double *host, int64_t n);
int  poro_vec_fill(poro_ctx *ctx, int which, double value);
int  poro_vec_copy(poro_ctx *ctx, int dst, int src);               /* e.g. old_solution = solution (PoroelasticityFSS.h:342) */
int  poro_vec_axpy(poro_ctx *ctx, int y, double a, int x);         /* solution += solution_update (:379)                    */
int  poro_vec_norm(poro_ctx *ctx, int which, double *l2, double *linf);

/* device-side snapshot of every PORO_VEC_* vector (one slot) and its restoration: lets a caller retry a time step (e.g. with another dt) or
 * repeat one for measurements without moving the state across PCIe; the reference has no counterpart (its only persistence is the per-step VTK dump,
 * PoroelasticityFSS.h:286-290). */
int  poro_state_save(poro_ctx *ctx);
int  poro_state_restore(poro_ctx *ctx);

/* PoroElasticDisplacementSolver<dim>::assemble_system (:155-291); pressure taken from PORO_VEC_P.
 * rebuild_matrix mirrors `rebuild_system_matrix` (:280): 1 = (re)build A_u (CSR values, or the
 * matrix-free operator data + diagonal) and the constant Dirichlet lifting, 0 = RHS only. */
int  poro_disp_assemble_system(poro_ctx *ctx, int rebuild_matrix);
/* PoroElasticDisplacementSolver<dim>::solve (:294-307): PCG, warm start from PORO_VEC_U, then constraints.distribute. */
int  poro_disp_solve(poro_ctx *ctx, const poro_solver_opts *opts, poro_solve_info *info);
/* 1 if `preconditioner` can be used by poro_pres_solve / poro_proj_solve (which_system = 1) or poro_disp_solve (which_system = 0) on this context, else 0.
 * which_system = 2: poro_proj_solve / poro_proj_solve_many alone (the mass matrix: prescribed pressures do not restrict it; they do restrict which_system = 1) */
int  poro_supports_preconditioner(poro_ctx *ctx, int32_t which_system, int32_t preconditioner);

/* PoroElasticPressureSolver<dim>::assemble_residual (:113-155) from PORO_VEC_{P,P_OLD,EPSV,EPSV0}; l2 = residual.l2_norm() (PoroelasticityFSS.h:364) */
int  poro_pres_assemble_residual(poro_ctx *ctx, double time_step, double *l2);
/* extension: PORO_VEC_P[dof] = value on the prescribed-pressure dofs of the descriptor; a no-op without any; call after setting the initial pressure (and after
 * poro_state_transfer_p).  On a context that also has hanging pressure nodes (cons_p) the pressure constraints are then distributed WITH their inhomogeneities,
 * p[h] = sum w p[master] + b, so that a hanging row with a prescribed master is conforming from the start: only updates are distributed afterwards, homogeneously,
 * and would carry a violation along for ever.  The prescribed dofs hold their listed values exactly.  Contexts without cons_p: unchanged, bit for bit. */
int  poro_pres_apply_boundary_values(poro_ctx *ctx);
/* PoroElasticPressureSolver<dim>::assemble_jacobian (:158-169) */
int  poro_pres_assemble_jacobian(poro_ctx *ctx, double time_step);
/* PoroElasticPressureSolver<dim>::solve (:172-185): J dp = R into PORO_VEC_DP (warm start) */
int  poro_pres_solve(poro_ctx *ctx, const poro_solver_opts *opts, poro_solve_info *info);
/* PoroElasticPressureSolver<dim>::update_volumetric_strain (:187-194): eps_v += (alpha/K) dp */
int  poro_pres_update_volumetric_strain(poro_ctx *ctx);

/* The pressure Newton loop of one fixed-stress iteration (PoroelasticityFSS.h:358-380) in one call:
 *   while (it < max_iterations) { ++it; update_volumetric_strain; assemble_residual; if (l2 < pressure_tol) break; assemble_jacobian; solve; p += dp; }   pinf = |p|_inf
 * enqueued as gated batches of iterations - a device-side test closes a gate where the per-call loop would have left, and every later kernel of the batch returns at once -
 * so that the host waits once per batch (normally once per call) instead of once per residual, check and norm.  The kernels of the per-call sequence in its order (p += dp
 * and the next iteration's strain update share a launch): every vector and every recorded number is what that sequence gives, bit for bit.
 * Eligible (poro_supports_pres_newton_loop): one rank, PORO_OP_MATRIX_FREE on a 3D box with the constant-coefficient pressure stencil (no per-cell permeability or moduli),
 * no hanging or prescribed pressure dofs, opts->preconditioner == PORO_PREC_FDM with the direct solve first (PORO_STOP_RHS).  PORO_PRES_HOST_LOOP in the environment when
 * the context is made: never eligible (A/B hook).
 * hint_slot (0..7, else none): which call of the time step this is; the length of the first batch comes from the count the same slot took last time.
 * record: iterations = residuals evaluated (= pressure_iteration), solves = direct solves whose check held, outcome PORO_NEWTON_*; l2[i] of iteration i + 1; res[k], bn[k]
 * of the k-th check (final and initial residual of that solve).  Arrays of max_iterations entries each, the caller's.
 * PORO_NEWTON_FALLBACK: the check of the direct solve of iteration `iterations` failed; PORO_VEC_DP holds the direct result, PORO_VEC_P is not yet updated, exactly the
 * state in which poro_pres_solve goes on to CG: the caller calls poro_pres_solve (which repeats the direct solve, same bits), updates p and runs the rest per call.
 * pinf is not set then.  The timer family "pressure_newton_batched" counts the calls with hint_slot == 0, that is the time steps whose loops ran this way (a count, no time). */
enum { PORO_NEWTON_CAP = 0, PORO_NEWTON_CONVERGED = 1, PORO_NEWTON_FALLBACK = 2 };
typedef struct poro_newton_record {
  int32_t iterations, solves, outcome, batches;
  double  pinf;
  double *l2, *res, *bn;
} poro_newton_record;
int  poro_supports_pres_newton_loop(poro_ctx *ctx, const poro_solver_opts *opts);
int  poro_pres_newton_loop(poro_ctx *ctx, double time_step, double pressure_tol, int32_t max_iterations, const poro_solver_opts *opts, int32_t hint_slot, poro_newton_record *record);

/* StrainProjector<dim>::assemble_projection_matrix (:101-106) */
int  poro_proj_assemble_matrix(poro_ctx *ctx);
/* StrainProjector<dim>::assemble_projection_rhs (:109-198); tensor_components are full indices a*dim+b */
int  poro_proj_assemble_rhs(poro_ctx *ctx, const int32_t *tensor_components, int32_t n_comp);
/* StrainProjector<dim>::solve_projection_system (:201-232); rhs_entry = packed symmetric entry */
int  poro_proj_solve(poro_ctx *ctx, int32_t rhs_entry, const poro_solver_opts *opts, poro_solve_info *info);
/* the loop of StrainProjector::solve_projection_system over several entries (PoroelasticityFSS.h:157-163) in one call: where PORO_PREC_FDM is the exact inverse of the
 * projection mass matrix the systems are solved directly and together (info[e].iterations = 0, residual checked against the stopping rule), otherwise entry by entry */
int  poro_proj_solve_many(poro_ctx *ctx, const int32_t *rhs_entries, int32_t n_entries, const poro_solver_opts *opts, poro_solve_info *info /* [n_entries] */);
/* PoroElasticProblem<dim>::get_volumetric_strain (PoroelasticityFSS.h:179-186): eps_v = sum of normal strains */
int  poro_get_volumetric_strain(poro_ctx *ctx);
/* PoroElasticProblem<dim>::get_effective_stresses (PoroelasticityFSS.h:189-224): sigma' = C : eps at every pressure node, C = isotropic_gassman_tensor
 * (ConstitutiveModel.h:45-57); PORO_VEC_STRAIN0+e -> PORO_VEC_STRESS0+e */
int  poro_get_effective_stresses(poro_ctx *ctx);

/* Mesh adaptation (refine_mesh, PoroelasticityFSS.h:447-498; appended entry points, no struct changes: PORO_ABI_VERSION stays 4).
 *
 * KellyErrorEstimator<dim>::estimate of PoroelasticityFSS.h:452-458 for the pressure-space vector `which_vec` (PORO_VEC_P, or any other vector of that space):
 * eta_host[n_cells], one indicator per cell.  THE DEFINITION BELOW IS THIS PROJECT'S (it follows deal.II's cell_diameter_over_24 strategy with coefficient 1 and an
 * empty Neumann map; deal.II itself was not available to compare against, so this text is what the tests pin):
 *   - for every interior face F shared by the cells K and K':  J_F = int_F [n . (grad p_h|_K - grad p_h|_K')]^2 dS, with the tensorised Gauss(2) rule on the face
 *     (QGauss<dim-1>(fe.degree + 1)) mapped with MappingQ1; surface element and normal from the face's own map (the convention of the Neumann term);
 *   - boundary faces contribute 0;
 *   - a hanging face is a coarse face of K against the 2^(dim-1) faces of its fine neighbours K'_s: one J_s per subface, integrated ON THE SUBFACE with Gauss(2), the
 *     coarse side's gradient evaluated at the matching reference points; the coarse cell receives the sum of the J_s, each fine neighbour its own J_s;
 *   - eta_K = sqrt(sum over the faces F of K of c_F J_F), c_F = h_K / 24 on regular faces and h_coarse / 24 for BOTH sides of a hanging face (deal.II takes the
 *     factor from the coarse cell); h = the cell diameter = the longest of the 2 (2D) or 4 (3D) vertex diagonals.
 * The face tables are built on the host at the first call (from the cells' pressure dofs, the boundary-face list and cons_p: a face of one cell only that is not in
 * the boundary-face list must pair with a coarse face through the masters of its hanging vertices - meshes with ONE level of hanging nodes; anything else returns
 * < 0 with a message) and stay on the device.  Two kernels, no atomics: the result is bitwise the same from call to call.  The call synchronises (it returns host
 * data), leaves every vector unchanged, works in both operator modes and on every single-rank mesh (box-tagged, tensor, refined, Gmsh; 2D and 3D); on a partitioned
 * context (n_ranks > 1) it returns < 0.  Timer family: "kelly". */
int  poro_pres_estimate_error(poro_ctx *ctx, int which_vec, double *eta_host /* [n_cells] */);
/* SolutionTransfer<dim>::interpolate of PoroelasticityFSS.h:474-497: PORO_VEC_P, PORO_VEC_EPSV, PORO_VEC_EPSV0 of `from` -> `to`, one launch:
 *   to[i] = sum_{k in ptr[i] .. ptr[i+1]} weight[k] * from[node[k]]   for every pressure dof i of `to` (the sum runs in the row's entry order).
 * The rows (ptr[to.n_dofs_p + 1], node, weight; host arrays) evaluate the old FE function at the new dofs; the host provider builds them for its refined boxes, a
 * caller with its own triangulation takes them from its SolutionTransfer.  They are checked on the host first (ptr[0] == 0, ptr ascending, nodes in range): a
 * malformed row, contexts on different devices or a partitioned context return < 0 and leave `to` untouched.  The launch is ordered after everything `from` has
 * enqueued and runs on `to`'s stream; the call returns when it has finished.  Every other vector of `to` is left as it is - zero on a new context, as after every
 * reinit of the reference (so the displacement warm start is lost across a refinement, as there).  Prescribed pressures of `to` are re-imposed by the caller with
 * poro_pres_apply_boundary_values. */
int  poro_state_transfer_p(poro_ctx *from, poro_ctx *to, const int64_t *ptr, const int32_t *node, const double *weight);

/* parity / measurement hooks */
int  poro_export_csr_size(poro_ctx *ctx, int which, int64_t *n_rows, int64_t *nnz);
int  poro_export_csr(poro_ctx *ctx, int which, int64_t *row_ptr, int32_t *col, double *val);
/* y = A x with the operator `which` (A_U honours the ctx operator mode); host in/out */
int  poro_apply_operator(poro_ctx *ctx, int which, const double *x_host, double *y_host);
/* z = P^-1 g with the displacement preconditioner (PORO_PREC_JACOBI | PORO_PREC_FDM), host in/out: parity hook for the preconditioner
 * PoroElasticDisplacementSolver<dim>::solve hands to cg.solve (:302-305; the reference's is PreconditionSSOR).  reps > 0 additionally times
 * `reps` applications on the device (HIP events) into *seconds_per_apply.
 * Partitioned contexts: PORO_PREC_FDM is COLLECTIVE - every rank calls it, each with its own window of g (its slab, shared planes included, the same values in both
 * copies of a shared plane), and gets its window of z; the set-up agrees on the form through all-reduces and every application runs two all-to-alls.  PORO_PREC_JACOBI
 * is local (the assembled diagonal already holds the neighbours' share on the shared planes). */
int  poro_apply_preconditioner_u(poro_ctx *ctx, int32_t preconditioner, const double *g_host, double *z_host, int32_t reps, double *seconds_per_apply);
/* repeat y = A_u x `reps` times on device-resident synthetic x; returns mean seconds per application (HIP events) */
int  poro_bench_operator(poro_ctx *ctx, int which, int operator_mode, int reps, double *seconds_per_apply);
/* accumulated HIP-event time (s) and launch count of the named kernel family since the last reset */
int  poro_timers_reset(poro_ctx *ctx);            /* clears the accumulators and switches event timing on */
int  poro_timers_enable(poro_ctx *ctx, int on);   /* 0: off; 1: events on every launch; k > 1: on every k-th launch of a family (the events cost ~2.5 us per launch), poro_timers_get scales the sampled time to all launches */
int  poro_timers_get(poro_ctx *ctx, const char *name, double *seconds, int64_t *launches);

/* Form of the block fast-diagonalisation preconditioner of the displacement system (PORO_PREC_FDM; appended entry points, no struct changes: PORO_ABI_VERSION stays 4).
 *   PORO_FDM_FORM_DEFAULT:       the octant form where every direction of a single-rank 3D box is mirror-symmetric for every component, else the nodal kernels.
 *   PORO_FDM_FORM_PER_DIRECTION: the octant form's three contiguous passes (g . z out of pass 2, the stopping test in pass 1, h and z in one array) where only SOME
 *                                directions are mirror-symmetric - a consolidation column held at the bottom and loaded at the top, a graded tensor-product grid.
 *                                Direction d is split in parity halves iff every component has the same condition at both of its ends and the eigenvectors of its line came
 *                                out even or odd; otherwise it keeps whole-length transforms.  A box whose directions are all split runs the octant form as always; one
 *                                with a transformed line of more than 128 entries keeps the nodal kernels.  fp64 transforms only: with PORO_FDM_FP32 requested as well,
 *                                poro_ctx_get_fdm_precision reports PORO_FDM_FP64.
 * Never chosen automatically.  The same mathematics in fp64: iteration counts within +-1 of the nodal kernels'.  Honoured by single-rank 3D contexts; partitioned
 * contexts, 2D and the coarse box of PORO_PREC_TWO_LEVEL record the request and run what they ran.  The environment variable PORO_FDMO_FORM=per-direction|default sets
 * the initial request of every context when it is created.
 * poro_ctx_set_fdm_form: any time between solves; a block FDM built in the other form is released and built again at its next use.  An unknown value is an error.
 * poro_ctx_get_fdm_form: `effective` = what PORO_PREC_FDM runs on this context, split[d] = 1 where direction d is split in parities.  It BUILDS the block FDM where the
 * context can use it (host eigenproblems, uploads, a stream synchronise), so that the answer is final: call it outside timed regions.  A context that cannot use
 * PORO_PREC_FDM on the displacement system, and a partitioned one before its first solve, report PORO_FDM_RUNS_NODAL.  split may be null.
 * The timer family "fdm_u_per_direction_form" counts the solves that ran the form. */
#define PORO_FDM_FORM_DEFAULT 0
#define PORO_FDM_FORM_PER_DIRECTION 1
enum { PORO_FDM_RUNS_NODAL = 0, PORO_FDM_RUNS_OCTANT = 1, PORO_FDM_RUNS_PER_DIRECTION = 2, PORO_FDM_RUNS_SLAB = 3, PORO_FDM_RUNS_PLANAR = 4 };
int  poro_ctx_set_fdm_form(poro_ctx *ctx, int32_t form);
int  poro_ctx_get_fdm_form(poro_ctx *ctx, int32_t *requested, int32_t *effective, int32_t split[3]);

/* Heterogeneous permeability: a per-cell k / mu for the pressure system (appended entry points, no struct changes: PORO_ABI_VERSION stays 4).
 * poro_ctx_set_cell_permeability: k_over_mu[n_cells], one value per cell in the descriptor's cell order, replaces poro_material.k_over_mu in the pressure residual, the
 * pressure Jacobian and poro_pres_solve: K_kappa = sum_c kappa_c K_c takes the place of kappa K.  NULL returns to the scalar; the residual and the Jacobian are then
 * bitwise what they were before a field was set.  The projection (mass matrix) and the displacement system are not affected.  ONE RANK ONLY: refused (< 0, poro_last_error
 * names the reason) on a partitioned context (n_ranks > 1), for a wrong n_cells and for a value that is not finite and > 0.  The call re-assembles the Laplace matrix and
 * invalidates the cached Jacobian (call poro_pres_assemble_jacobian again), the ILU factor and the cached factors of the line solve below.
 * poro_ctx_get_cell_permeability: kind = 0 no field; 1 a field that is constant (exact equality) within every cell layer of the SLOWEST direction of a uniform box or
 * tensor-product grid (kappa(z) in 3D, kappa(y) in 2D); 2 any other field.  out (may be NULL) receives the values, n_cells as in the setter.
 * Preconditioners of poro_pres_solve while a field is set (poro_supports_preconditioner(ctx, 1, ...) tells): PORO_PREC_JACOBI / NONE / ILU0 / SSOR as without one.
 * PORO_PREC_FDM on uniform boxes and tensor-product grids, with or without whole prescribed faces: x (and y) transforms with the constant-coefficient eigenpairs, then one
 * SPD tridiagonal solve per mode along the slowest direction, (a Mz + Kz^kappa + (lam_x + lam_y) Mz^kappa) t = r, then back.  kind 1: the exact inverse - a direct solve
 * on matrix-free boxes (info.iterations = 0), the preconditioner of CG on tensor grids and CSR contexts.  kind 2: the same form built from the arithmetic layer means
 * preconditions CG; never a direct solve (a field layered along another direction is of this kind: its layer means are one constant).  PORO_PREC_TWO_LEVEL is refused
 * for the pressure system while a field is set: the coarse box is a constant-coefficient context.
 * Exports with a field set: poro_export_csr(PORO_MAT_LAPLACE_P) returns K_kappa (the scalar is not applied), PORO_MAT_JACOBIAN_P returns M / (M_b dt) + K_kappa. */
int  poro_ctx_set_cell_permeability(poro_ctx *ctx, const double *k_over_mu /* NULL: back to the scalar */, int64_t n_cells);
int  poro_ctx_get_cell_permeability(poro_ctx *ctx, double *out /* may be NULL */, int64_t n_cells, int32_t *kind);
/* parity hook: y = J x with the operator the Krylov solver of poro_pres_solve applies - the (variable-coefficient) stencil on matrix-free boxes, the CSR Jacobian elsewhere;
 * without condensation and with the prescribed rows in place.  After poro_pres_assemble_jacobian; host in/out */
int  poro_pres_apply_jacobian(poro_ctx *ctx, const double *x_host, double *y_host);

/* Heterogeneous elastic moduli: a per-cell Lame lambda and shear modulus G for the displacement system (appended entry points, no struct changes: PORO_ABI_VERSION stays 4).
 * poro_ctx_set_cell_moduli: lame_lambda[n_cells], shear_G[n_cells], one pair per cell in the descriptor's cell order, replace poro_material.lame_lambda / shear_G wherever the
 * displacement system reads them: the general matrix-free cell kernels (both scatter modes, operator and diagonal), the coloured CSR assembly (so PORO_MAT_A_U, the SpMV, SSOR
 * and ILU0 follow), the lifting of the Dirichlet values, poro_apply_operator and PORO_VEC_DIAG_U.  Both NULL returns to the scalars: results are then bitwise what they were
 * before a field was set.  One NULL is refused.  ONE RANK ONLY: refused (< 0, poro_last_error names the reason) on a partitioned context (n_ranks > 1), on a context in
 * PORO_OPFORM_HYBRID, for a wrong n_cells and for a cell whose values are not finite with G > 0 and 3 lambda + 2 G > 0 (the message names the cell).
 * The call drops the assembled matrix, the Jacobi diagonal and its dictionary, the lifting vector, the element matrix, the Chebyshev eigenvalue estimate, the ILU factor and
 * the FDM tables of the displacement system: call poro_disp_assemble_system next - it rebuilds whatever its rebuild flag says.
 * Box-tagged contexts with a field: the structured kernels and the single element matrix are constant-coefficient, so operator, diagonal, lifting and the CSR assembly take the
 * general cell loop (several times slower per application); PORO_PREC_CHEBYSHEV runs its unfused recurrence.  The coupling right-hand side, the pressure stencils
 * and the projection do not depend on the moduli and keep their kernels.  poro_ctx_set_scatter_mode is honoured on such a box.
 * Preconditioners of poro_disp_solve while a field is set (poro_supports_preconditioner(ctx, 0, ...) tells): PORO_PREC_JACOBI / CHEBYSHEV / NONE everywhere, ILU0 / SSOR on the
 * assembled operator.  PORO_PREC_FDM on uniform boxes and tensor-product grids whose Dirichlet sets it accepts without a field: the x (and y) transforms with the eigenpairs of
 * every (component, direction), then one SPD banded solve per component and mode along the slowest direction (tridiagonal for Q1, pentadiagonal for Q2; the factorisation is
 * cached per field, (k_u + 1) n_u doubles), then back.  kind 1: the exact inverse of the block diagonal; kind 2: the same form built from the arithmetic layer means of lambda
 * and G, a preconditioner.  With a field only the nodal tables are built: poro_ctx_set_fdm_precision, poro_ctx_set_fdm_form and the PORO_FDMO_* / PORO_FDMU_SINGLE switches
 * are ignored (the getters report PORO_FDM_FP64 / PORO_FDM_RUNS_NODAL).  PORO_PREC_TWO_LEVEL is refused (the coarse box is a constant-coefficient context) and so is
 * PORO_OPFORM_HYBRID, also the other way round: a context in the hybrid form refuses the field.
 * poro_get_effective_stresses and poro_pres_update_volumetric_strain (K = lambda + 2 G / 3) then use NODAL moduli: at a pressure dof the arithmetic mean over the cells that
 * touch it - the layer's value inside a layer, the mean on an interface.
 * poro_ctx_get_cell_moduli: kind = 0 no field; 1 both arrays constant (exact equality) within every cell layer of the SLOWEST direction of a uniform box or tensor-product
 * grid; 2 any other field.  lambda_out / G_out (each may be NULL) receive the values, n as n_cells in the setter. */
int  poro_ctx_set_cell_moduli(poro_ctx *ctx, const double *lame_lambda, const double *shear_G /* both NULL: back to the scalars */, int64_t n_cells);
int  poro_ctx_get_cell_moduli(poro_ctx *ctx, double *lambda_out, double *G_out /* may be NULL */, int64_t n, int32_t *kind);

/* Anisotropic permeability: a per-cell DIAGONAL tensor kappa_c = diag(kx, ky[, kz]) / mu whose principal axes are the global coordinate axes (appended entry points, no
 * struct changes: PORO_ABI_VERSION stays 4).  K_kappa = sum_c int_c grad(phi_i) . kappa_c grad(phi_j) takes the place of kappa K wherever poro_ctx_set_cell_permeability
 * puts its scalar field: the residual, the Jacobian, poro_pres_apply_jacobian, poro_pres_solve, the exports (PORO_MAT_LAPLACE_P = K_kappa, PORO_MAT_JACOBIAN_P =
 * M / (M_b dt) + K_kappa).  k_over_mu[n_cells][dim], x first, cells in the descriptor's order.
 * A context holds the scalar field OR the tensor: setting one drops the other, NULL to either setter returns to poro_material.k_over_mu (bitwise, as above).  While a tensor
 * is set poro_ctx_get_cell_permeability reports the tensor's kind and refuses a non-NULL out.  Refusals and invalidations as for the scalar field: ONE RANK ONLY, a wrong
 * n_cells, a component that is not finite and > 0 (the message names the cell and the component); a refused call leaves the context as it was.
 * kind = 0 no tensor; 1 EVERY component constant (exact equality) within every cell layer of the slowest direction of a uniform box or tensor-product grid; 2 anything else.
 * PORO_PREC_FDM stays exact for kind 1: in the eigenbasis of the leading directions one SPD tridiagonal system per mode is left,
 * (a Mz + lam_x Mz^kx + lam_y Mz^ky + Kz^kz) t = r  (2D: (a My + lam_x My^kx + Ky^ky) t = r) - a direct solve on matrix-free boxes (info.iterations = 0), the
 * preconditioner of CG on tensor grids and CSR contexts; kind 2: the same form with per-component arithmetic layer means, never claimed exact.  PORO_PREC_TWO_LEVEL is
 * refused for the pressure system; the other preconditioners as without a field. */
int  poro_ctx_set_cell_permeability_tensor(poro_ctx *ctx, const double *k_over_mu /* [n_cells][dim], x first; NULL: back to the scalar */, int64_t n_cells);
int  poro_ctx_get_cell_permeability_tensor(poro_ctx *ctx, double *out /* [n_cells][dim], may be NULL */, int64_t n_cells, int32_t *kind);

/* Form of the displacement operator on a box with per-cell moduli (appended entry points, no struct changes: PORO_ABI_VERSION stays 4).
 *   PORO_MODULI_OP_CELLS:      the general cell loop, as poro_ctx_set_cell_moduli describes (the default).
 *   PORO_MODULI_OP_STRUCTURED: one structured launch per application where lambda and G are constant within every cell layer of z (kind 1): the operator is still a sum of
 *                              Kronecker products of 1D matrices whose z factor carries the weight.  The same mathematics in another summation order: results
 *                              agree with the cell loop to rounding (1e-12 of max|y|), not bitwise; bitwise reproducible from run to run.
 * Never chosen automatically.  The request may be made at any time and stays through field changes.  It is EFFECTIVE on a single-rank box-tagged (uniform) 3D context of
 * degree 1 or 2 in PORO_OP_MATRIX_FREE mode with the sum-factorised variant while a kind-1 field is set; everywhere else - no field, a kind-2 field, 2D, tensor-product
 * grids without the box tag, refined meshes, PORO_OP_CSR - the request is recorded and the context runs exactly what it ran.  While effective, the operator of
 * poro_disp_solve (with the fused x . y), the Chebyshev recurrence, poro_apply_operator and poro_bench_operator take the structured kernel; the scatter mode is stored and
 * reported but not used.  The Jacobi diagonal, the lifting and the CSR assembly keep the cell loop (once per field or assembly).
 * The environment variable PORO_MODULI_OPERATOR=structured|cells sets the initial request of every context when it is created.
 * poro_ctx_get_moduli_operator: `effective` = what an application runs now.  An unknown form is an error. */
enum { PORO_MODULI_OP_CELLS = 0, PORO_MODULI_OP_STRUCTURED = 1 };
int  poro_ctx_set_moduli_operator(poro_ctx *ctx, int32_t form);
int  poro_ctx_get_moduli_operator(poro_ctx *ctx, int32_t *requested, int32_t *effective);

/* Gravity: body force and Darcy gravity flux (appended entry points, no struct changes: PORO_ABI_VERSION stays 4).  Off by default - the reference's body force is
 * identically zero and that stays the parity definition.  With a gravity vector g, bulk density rho_b (one scalar, or one value per cell) and fluid density
 * rho_f:
 *   displacement right-hand side   b_i += sum_c rho_b,c int_c g . phi_i                                   (beside the tractions)
 *   Darcy's law                    q = -kappa (grad p - rho_f g), so the pressure residual becomes R = -((M t + kappa K p) + (src + f_g)),
 *                                  f_g[i] = -sum_c rho_f int_c (kappa_c g) . grad(phi_i),  kappa_c = poro_material.k_over_mu, the per-cell k / mu or its diagonal tensor
 *                                  (kappa_c g componentwise), whichever the context holds.  For p = rho_f g . x + const the flux part of R vanishes on every row.
 * Both vectors are constant in time: they are built when a setting changes and summed into constant vectors the time step reads anyway (the traction vector; the source
 * vector of the residual), so a step costs what it cost, and without gravity every result is bitwise what it was.  PORO_VEC_SOURCE_P keeps meaning the well alone.
 * poro_ctx_set_gravity: g is [dim]; NULL or all zeros switches gravity off (the earlier bits come back).  bulk_density: the scalar rho_b (>= 0); fluid_density: rho_f
 *   (>= 0; 0: no flux term).  Any time; the next poro_disp_assemble_system rebuilds the load vector alone (not the matrix, the diagonal, the lifting or the tables of
 *   PORO_PREC_FDM) whatever its rebuild_matrix says, the next poro_pres_assemble_residual reads the new flux.  Works on slab and general partitions: both vectors are the
 *   rank's partial sums over its cells, completed by the interface sums of the right-hand side and of the residual.
 * poro_ctx_set_cell_density: rho[n_cells] > 0 in the descriptor's cell order replaces the scalar rho_b (NULL: back to it).  One rank only.  A refused call (wrong count, a
 *   value that is not finite and > 0 - the message names the cell) leaves the context as it was.  `kind` of the getter as for the other per-cell fields.
 * poro_get_gravity_vectors: the two vectors alone, without tractions and well (zeros while off); either pointer may be NULL. */
int  poro_ctx_set_gravity(poro_ctx *ctx, const double *g /* [dim] or NULL */, double bulk_density, double fluid_density);
int  poro_ctx_get_gravity(poro_ctx *ctx, double *g /* [dim], may be NULL */, double *bulk_density, double *fluid_density, int32_t *on);
int  poro_ctx_set_cell_density(poro_ctx *ctx, const double *rho /* [n_cells], NULL: back to the scalar */, int64_t n_cells);
int  poro_ctx_get_cell_density(poro_ctx *ctx, double *out /* [n_cells], may be NULL */, int64_t n_cells, int32_t *kind);
int  poro_get_gravity_vectors(poro_ctx *ctx, double *body_u /* [n_dofs_u] or NULL */, double *flux_p /* [n_dofs_p] or NULL */);

/* Darcy velocity, boundary discharge and fluid mass balance (appended entry points, no struct of the existing ABI changes: PORO_ABI_VERSION stays 4).  Pure
 * post-processing: the calls synchronise (they return host data), leave every PORO_VEC_* vector unchanged, work in both operator modes and on every single-rank mesh
 * (box-tagged, tensor, refined with hanging nodes, Gmsh; 2D and 3D) and read the permeability and the gravity the context holds AT THE TIME OF THE CALL.  A vector that
 * is not in the pressure space, a partitioned context (n_ranks > 1) and time_step <= 0 return < 0 with a message.  Timer families: "darcy", "flow_balance"
 * (inside them, for measurements: "darcy_bfaces", "darcy_label_sums", "flow_balance_sums" bracket those kernels alone).
 * THE DEFINITIONS BELOW ARE THIS PROJECT'S (the reference computes no flow); this text is what the tests pin.
 *   kappa_c = what the context holds for cell c: poro_material.k_over_mu, the per-cell k / mu, or its per-cell diagonal tensor (products then componentwise).
 *   rho_f g = the gravity term of Darcy's law; zero unless gravity is on with a fluid density - exactly the condition under which the residual carries the gravity flux.
 * Cell velocity (poro_pres_darcy_velocity): q_c = -kappa_c (grad p_h(x_c) - rho_f g), p_h the Q1 function of the pressure-space vector `which_vec`, x_c the image of
 *   the reference centre (1/2, ..., 1/2) under MappingQ1.  q_host[n_cells][dim], cells in the descriptor's order.
 * Face discharge (poro_pres_boundary_discharge): for entry b of the boundary-face list (local face f = 2 d + side of its cell)
 *   Q_b = int_F q . n dS with the tensorised Gauss(2) rule on the face, q = -kappa_c (grad p_h - rho_f g) evaluated from the face's own cell at the face points, n dS
 *   from the face's own map (column d of det(J) J^-T with the sign of the side: the convention of the Neumann term and of the Kelly indicator).  n is outward: positive
 *   means fluid leaving.  Q_face_host[n_bfaces] (may be NULL).
 * Label sums: Q_label_host[l] = the sum of Q_b over the faces with bface_id == labels[l], in list order per lane (a fixed face-to-lane assignment and a fixed-order
 *   block sum: no float atomics, the same bits from call to call); a label no face carries gives exactly 0.  labels may be NULL with n_labels = 0.
 * Discrete balance (poro_pres_flow_balance): let r = M t + kappa K p + src be the pressure residual's own vector before any sign, condensation or masking,
 *   t = alpha (eps_v - eps_v0) / dt + (p - p_old) / (M_b dt) from PORO_VEC_{EPSV, EPSV0, P, P_OLD}, src what poro_pres_assemble_residual uses (the well alone, or well
 *   plus gravity flux), Rt = C^T(-r) the condensed residual BEFORE the prescribed rows are zeroed, and m_j = sum_i M_ij = int phi_j the lumped mass (built once per
 *   context from its own mass matrix).  Reported:
 *     storage_rate_strain   = sum_j m_j alpha (eps_v - eps_v0)_j / dt
 *     storage_rate_pressure = sum_j m_j (p - p_old)_j / (M_b dt)
 *     source_sum            = sum_i src_i   (negative for an injecting well)
 *     outflow_prescribed    = sum of Rt_i over the prescribed-pressure rows: since -r_i = int_Gamma phi_i q . n there, the conservative discharge through the drained boundary
 *     free_row_sum          = sum of Rt_i over all other rows
 *     residual_l2           = sqrt(sum over the other rows of Rt_i^2), the number poro_pres_assemble_residual returns
 *   and optionally Rt_i for every prescribed dof in the order of poro_desc.dirichlet_dof_p (outflow_dof_host[n_dirichlet_p]).  Algebraic identity, on every mesh and with
 *   every permeability form (the columns of K sum to zero, the gravity flux vector sums to zero, hanging-node weights sum to one):
 *     outflow_prescribed + free_row_sum = -(storage_rate_strain + storage_rate_pressure + source_sum).
 *   |free_row_sum| <= sqrt(n_dofs_p) residual_l2 (Cauchy-Schwarz): a step whose pressure loop converged closes its balance to sqrt(n_dofs_p) * its tolerance.
 *   CAVEAT: with the reference's loop as committed (storage against the eps_v0 of the run's START) storage_rate_strain is the discrete system's term, not a physical
 *   rate; it is physical where eps_v0 is the previous step's strain (the host layer's incremental_strain switch).
 *   Rt is assembled into scratch by the calls poro_pres_assemble_residual makes; PORO_VEC_RESIDUAL_P is not touched. */
typedef struct poro_flow_balance_terms { double storage_rate_strain, storage_rate_pressure, source_sum, outflow_prescribed, free_row_sum, residual_l2; } poro_flow_balance_terms;
int  poro_pres_darcy_velocity(poro_ctx *ctx, int which_vec, double *q_host /* [n_cells][dim] */);
int  poro_pres_boundary_discharge(poro_ctx *ctx, int which_vec, double *Q_face_host /* [n_bfaces] or NULL */, const int32_t *labels, int32_t n_labels, double *Q_label_host /* [n_labels] or NULL */);
int  poro_pres_flow_balance(poro_ctx *ctx, double time_step, poro_flow_balance_terms *out, double *outflow_dof_host /* [n_dirichlet_p] or NULL */);

/* Cell stresses, failure measures and support reactions (appended entry points, no struct of the existing ABI changes: PORO_ABI_VERSION stays 4).  Pure post-processing,
 * the mechanical twin of the flow calls above: the calls synchronise (they return host data), leave every PORO_VEC_* vector unchanged, work in both operator modes and on
 * every single-rank mesh (box-tagged, tensor, refined with hanging nodes, Gmsh; 2D and 3D; Q1 and Q2 displacements).  A partitioned context (n_ranks > 1), a vector of the
 * wrong space, a friction angle outside [0, pi/2) and a cohesion < 0 return < 0 with a message.  Timer families: "cell_stress", "cell_measures", "force_balance".
 * THE DEFINITIONS BELOW ARE THIS PROJECT'S (the reference computes none of this); this text is what the tests pin.
 *   Sign: tension is positive, as in sigma' = C : eps everywhere in the code.
 *   Packed symmetric order: the one of PORO_VEC_STRAIN0 + e - 2D: xx, xy, yy; 3D: xx, xy, xz, yy, yz, zz.
 *   lambda_c, G_c = what the context holds for cell c AT THE TIME OF THE CALL: the scalars of poro_material, or the cell's own pair of poro_ctx_set_cell_moduli - never a
 *   nodal mean (poro_get_effective_stresses multiplies by nodal means and is left as it is).  alpha = mat.biot_alpha.  u_h = the FE_Q(k)^dim function of a
 *   displacement-space vector, p_h = the Q1 function of a pressure-space vector, x_c = the image of the reference centre (1/2, ..., 1/2) under MappingQ1 - the point of
 *   poro_pres_darcy_velocity, so the cell data are co-located.
 * Cell stress (poro_disp_cell_stress):
 *   eps_c    = sym grad u_h(x_c), from the cell's own dofs and the true J^-1 at the centre (non-affine cells included)
 *   sigma'_c = lambda_c tr(eps_c) I + 2 G_c eps_c
 *   sigma_c  = sigma'_c - alpha p_h(x_c) I;   which_p = -1: no pressure, sigma = sigma'
 *   Each output is [n_cells][n_sym], cells in the descriptor's order, and may be NULL.
 * Cell measures (poro_disp_cell_measures): from the 3 x 3 EFFECTIVE stress.  In 2D that is plane strain: the in-plane block plus sigma'_zz = lambda_c tr(eps_c), which can
 *   be the largest, the middle or the smallest principal value.  measures_host[n_cells][6] (may be NULL): s1 >= s2 >= s3 (principal effective stresses), the mean tr / 3,
 *   von Mises sqrt(3 J2), and the Mohr-Coulomb function f = (s1 - s3) / 2 + (s1 + s3) / 2 * sin(phi) - c * cos(phi); f >= 0: the envelope is reached.
 *   mc = {cohesion c >= 0, friction angle phi in radians, 0 <= phi < pi/2}; mc = NULL: f = 0 and a summary of zeros.
 *   summary (may be NULL) = {max_f, argmax_cell, n_failing = the number of cells with f >= 0}, computed on the device in fixed order (per-block partials, finished in one
 *   block; a tie goes to the lowest cell index; no float atomics: the same bits from call to call).
 *   which_p must be -1 or a pressure-space vector and is otherwise IGNORED: the measures are those of the effective stress (one signature for both calls).
 *   The eigenvalues come from a fixed number of cyclic Jacobi sweeps (csrc/stress_measures.hpp): accurate for repeated and nearly repeated principal stresses.
 * Force balance (poro_disp_force_balance): let b = b_cpl + b_neu + b_body be the three parts of the displacement right-hand side on ALL rows, without Dirichlet masking
 *   and without lifting: b_cpl,i = alpha int p_h div(phi_i) with the current PORO_VEC_P, b_neu = the Neumann (traction) vector, b_body = the gravity body force or zero;
 *   r = A_full u - b with A_full the unconstrained operator (the one the lifting is built with) and u = PORO_VEC_U; Rt = C^T r the residual condensed through cons_u
 *   (hanging nodes, rigid-plate ties) BEFORE the Dirichlet rows are touched.  Per component k < dim (arrays of 3, unused entries 0; the component of a dof is its local
 *   index s * dim + comp in cell_dofs_u, tabulated once per context):
 *     reaction_sum[k] = sum of Rt_i over the Dirichlet rows of component k: the force the supports exert on the body.  One addition keeps this complete on meshes whose
 *                       hanging nodes lie on a supported face: the host provider closes its lists, i.e. a hanging row h whose masters are prescribed no longer names them
 *                       and its weights sum to less than one.  The share (1 - sum_m w_hm) r_h that those masters' rows would have received is added to the sum of its
 *                       component (it is exactly 0.0 for every other row and for every tie).  reaction_dof_host cannot attribute it to a dof and leaves it out
 *     free_row_sum[k] = sum of Rt_i over all other rows of component k
 *     traction_sum[k] = sum over the component-k rows of b_neu,i;   body_sum[k] = ... of b_body,i;   coupling_sum[k] = ... of b_cpl,i
 *     residual_l2     = the 2-norm of Rt over the non-Dirichlet rows
 *   Identity (the shape functions of one component sum to one, so the component-k rows of A_full sum to zero; it holds wherever every constraint row has masters of
 *   its own component and weights that sum to one - or to less than one only because prescribed masters were eliminated, see reaction_sum - which covers every list the
 *   host provider builds):
 *     reaction_sum[k] + free_row_sum[k] = -(traction_sum[k] + body_sum[k] + coupling_sum[k]),
 *   coupling_sum[k] itself being zero to rounding (it is alpha int p d_k(1)).  |free_row_sum[k]| <= sqrt(n_dofs_u) residual_l2: the supports of a converged step carry
 *   exactly the applied load.  reaction_dof_host (optional) receives Rt_i for every Dirichlet dof in the order of poro_desc.dirichlet_dof.
 *   Everything is assembled in scratch: PORO_VEC_RHS_U and every other vector are untouched. */
typedef struct poro_mohr_coulomb { double cohesion, friction_angle /* radians */; } poro_mohr_coulomb;
typedef struct poro_failure_summary { double max_f; int64_t argmax_cell, n_failing; } poro_failure_summary;
typedef struct poro_force_balance_terms { double reaction_sum[3], free_row_sum[3], traction_sum[3], body_sum[3], coupling_sum[3], residual_l2; } poro_force_balance_terms;
int  poro_disp_cell_stress(poro_ctx *ctx, int which_u, int which_p /* -1: none */, double *strain_host, double *stress_eff_host, double *stress_tot_host /* [n_cells][n_sym] each, or NULL */);
int  poro_disp_cell_measures(poro_ctx *ctx, int which_u, int which_p /* -1 or a pressure-space vector; ignored */, const poro_mohr_coulomb *mc /* or NULL */,
                             double *measures_host /* [n_cells][6] or NULL */, poro_failure_summary *summary /* or NULL */);
int  poro_disp_force_balance(poro_ctx *ctx, poro_force_balance_terms *out, double *reaction_dof_host /* [n_dirichlet] or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* POROEL_HIP_H */
