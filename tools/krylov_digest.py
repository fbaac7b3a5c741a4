"""One line per Krylov solve path: return codes, iteration counts, operator applications and the SHA-256 of the solution, on the smallest shapes that reach every branch of
the three drivers (device-controlled PCG, its single-reduction form, the host-driven form) and of the preconditioner contract.  Every case solves its system twice: from a
zero start to a loose tolerance, then warm to the tight one, so that the second solve runs on the iteration-count hint of the first.  Two commits whose outputs are equal line
for line compute the same bits and take the same number of iterations there.

    python tools/krylov_digest.py                    every variant, one fresh child process each (some switches are read once per process), stopping at the first failure
    python tools/krylov_digest.py --variant NAME     the cases of one variant in this process, under whatever environment the caller set"""
import hashlib, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path[:0] = [ROOT]
import numpy as np
import poroelasticity_dealii_amd as pk
import bench

BC_2D, BC_3D = bench.BC_3D[:4], bench.BC_3D
MF, CSR = pk.OP_MATRIX_FREE, pk.OP_CSR
# meshes: box = (cells, degree, Dirichlet list), refined = (cells, degree, first refined cell, one past the last); the box shapes are those of tools/fdm_digest.py
BOXES = {"oct_q2": ((3, 4, 5), 2, BC_3D),               # 2079 displacement dofs: the odd tail of the 16-byte update kernels
         "nodal_full": ((3, 4, 5), 2, [(0, 0, 0.0), (2, 1, 0.0), (4, 2, 0.0)]),
         "planar_split": ((5, 7), 2, BC_2D),
         "q1_2d": ((5, 7), 1, BC_2D),
         "q1_3d": ((9, 5, 2), 1, BC_3D)}
REFINED = {"refined_2d": ((4, 3), 2, (1, 1), (3, 2)), "refined_3d": ((3, 3, 2), 2, (1, 1, 0), (2, 2, 1))}
# displacement cases: name -> (mesh, operator mode, preconditioner, disp_solve keywords, fp32 transforms, environment of the case)
U_CASES = {"u_jacobi_mf": ("oct_q2", MF, pk.PREC_JACOBI, {}, False, {}),                 # dictionary diagonal, fused d.h
           "u_jacobi_csr": ("q1_2d", CSR, pk.PREC_JACOBI, {}, False, {}),                # full diagonal, separate dot
           "u_jacobi_hanging": ("refined_2d", MF, pk.PREC_JACOBI, {}, False, {}),        # the condensing branch of the operator
           "u_chebyshev_mf": ("oct_q2", MF, pk.PREC_CHEBYSHEV, {"poly_degree": 4}, False, {}),
           "u_chebyshev_csr": ("q1_2d", CSR, pk.PREC_CHEBYSHEV, {"poly_degree": 4}, False, {}),
           "u_fdm_oct": ("oct_q2", MF, pk.PREC_FDM, {}, False, {}),
           "u_fdm_oct_fp32": ("oct_q2", MF, pk.PREC_FDM, {}, True, {}),
           "u_fdm_planar": ("planar_split", MF, pk.PREC_FDM, {}, False, {}),
           "u_fdm_nodal": ("nodal_full", MF, pk.PREC_FDM, {}, False, {}),
           "u_fdm_no_oct": ("oct_q2", MF, pk.PREC_FDM, {}, False, {"PORO_FDMU_NO_OCT": "1"}),
           "u_two_level": ("refined_3d", MF, pk.PREC_TWO_LEVEL, {}, False, {}),
           "u_ssor": ("q1_2d", CSR, pk.PREC_SSOR, {}, False, {}),
           "u_ilu0": ("q1_2d", CSR, pk.PREC_ILU0, {}, False, {})}
# pressure + projection cases: name -> (mesh, operator mode, preconditioner, tight relative tolerance)
Q1_CASES = {"q1_jacobi": ("q1_3d", MF, pk.PREC_JACOBI, 1e-13), "q1_fdm": ("q1_3d", MF, pk.PREC_FDM, 1e-8), "q1_ssor": ("q1_3d", CSR, pk.PREC_SSOR, 1e-12),
            "q1_ilu0": ("q1_3d", CSR, pk.PREC_ILU0, 1e-12), "q1_two_level": ("refined_3d", MF, pk.PREC_TWO_LEVEL, 1e-13)}
PARTITIONED = ["u_jacobi_mf", "u_chebyshev_mf", "u_fdm_oct", "u_fdm_no_oct", "q1_jacobi", "q1_fdm"]
ONE_RANK = {"PORO_FORCE_PARTITIONED_PATH": "1"}     # the partitioned code path on one rank with RCCL as the communicator (tools/partitioned_path_1rank.py)
VARIANTS = {"default": ({}, [k for k in U_CASES if k != "u_fdm_no_oct"] + list(Q1_CASES)),
            "separate_buffers": ({"PORO_FDMO_SEPARATE_BUFFERS": "1"}, ["u_fdm_oct", "u_fdm_oct_fp32"]),
            "separate_gz": ({"PORO_FDMO_SEPARATE_GZ": "1"}, ["u_fdm_oct", "u_fdm_oct_fp32", "u_fdm_planar"]),
            "cheb_unfused": ({"PORO_CHEB_UNFUSED": "1"}, ["u_chebyshev_mf"]),
            "iterative_q1": ({"PORO_PRES_ITERATIVE": "1", "PORO_PROJ_ITERATIVE": "1"}, ["q1_fdm"]),     # Q1 FDM through pcg with the explicit preconditioner
            "partitioned": (ONE_RANK, PARTITIONED),
            "partitioned_two_reductions": (dict(ONE_RANK, PORO_TWO_REDUCTION_CG="1"), PARTITIONED),
            "partitioned_iterative_q1": (dict(ONE_RANK, PORO_PRES_ITERATIVE="1", PORO_PROJ_ITERATIVE="1"), ["q1_fdm"])}   # the single-reduction driver with an explicit Q1 preconditioner


def problem(mesh):
    if mesh in BOXES:
        n, deg, bc = BOXES[mesh]
        return pk.Problem.box(len(n), list(n), [10.0] * len(n), deg, bench.material(), bc)
    n, deg, lo, hi = REFINED[mesh]
    return pk.Problem.refined_box(len(n), list(n), [10.0] * len(n), deg, bench.material(), BC_2D if len(n) == 2 else BC_3D, list(lo), list(hi))


def context(P, mode):
    G = pk.Context(P, 0, mode)
    if "PORO_FORCE_PARTITIONED_PATH" in os.environ:
        G.comm_rccl(pk.rccl_unique_id())
    return G


def u_inputs(n_p):
    return bench.INPUT["p_init"] * (1 + 0.3 * np.sin(0.37 * np.arange(n_p)))


def q1_inputs(n_p, n_u):
    """(vector -> values) of the pressure residual's inputs, and the displacement the projection's right-hand sides are assembled from"""
    p0, i, j = bench.INPUT["p_init"], np.arange(n_p), np.arange(n_u)
    vals = {pk.VEC_P: p0 * (1 + 0.3 * np.sin(0.37 * i)), pk.VEC_P_OLD: p0 * (1 + 0.1 * np.cos(0.21 * i)), pk.VEC_EPSV: 1e-6 * np.sin(0.13 * i), pk.VEC_EPSV0: np.zeros(n_p)}
    return vals, 1e-5 * np.sin(0.37 * j) + 1e-6 * np.cos(0.05 * j)


def proj_entries(dim):
    return [0, 2] if dim == 2 else [0, 3, 5]


def run_u(name, P):
    """-> (return codes, infos, solution) of the two solves of a displacement case"""
    mesh, mode, prec, kw, fp32, env = U_CASES[name]
    os.environ.update(env)
    G = context(P, mode)
    try:
        if fp32:
            G.set_fdm_precision(pk.FDM_FP32)
        G.set(pk.VEC_P, u_inputs(G.n_p)); G.disp_assemble_system(True)
        G.fill(pk.VEC_U, 0.0)
        rc0, i0 = G.disp_solve(abs_tol=1e-14, rel_tol=1e-6, max_iter=20000, prec=prec, **kw)
        rc1, i1 = G.disp_solve(abs_tol=1e-14, rel_tol=1e-11, max_iter=20000, prec=prec, **kw)
        return [rc0, rc1], [i0, i1], G.get(pk.VEC_U)
    finally:
        G.close()
        for k in env:
            del os.environ[k]


def run_q1(name, P):
    """-> per system (pressure, projection): (return codes, infos, solution); the projection's three normal strains are solved in one call and concatenated"""
    mesh, mode, prec, tol = Q1_CASES[name]
    G = context(P, mode)
    try:
        vals, u = q1_inputs(G.n_p, G.n_u)
        for k, v in vals.items():
            G.set(k, v)
        dt = bench.INPUT["dt"]
        G.pres_assemble_residual(dt); G.pres_assemble_jacobian(dt); G.fill(pk.VEC_DP, 0.0)
        rc0, i0 = G.pres_solve(rel_tol=max(tol, 1e-6), max_iter=5000, prec=prec)
        rc1, i1 = G.pres_solve(rel_tol=tol, max_iter=5000, prec=prec)
        pres = ([rc0, rc1], [i0, i1], G.get(pk.VEC_DP))
        ents = proj_entries(G.dim)
        G.set(pk.VEC_U, u); G.proj_assemble_matrix(); G.proj_assemble_rhs([a * G.dim + a for a in range(G.dim)])
        for e in ents:
            G.fill(pk.VEC_STRAIN0 + e, 0.0)
        rc0, j0 = G.proj_solve_many(ents, rel_tol=max(tol, 1e-6), max_iter=5000, prec=prec)
        rc1, j1 = G.proj_solve_many(ents, rel_tol=tol, max_iter=5000, prec=prec)
        return pres, ([rc0, rc1], j0 + j1, np.concatenate([G.get(pk.VEC_STRAIN0 + e) for e in ents]))
    finally:
        G.close()


def line(variant, case, rcs, infos, x):
    sha = hashlib.sha256(np.ascontiguousarray(x, dtype=np.float64).tobytes()).hexdigest()
    lst = lambda v: ",".join(str(int(a)) for a in v)
    return f"{variant} {case} rc={lst(rcs)} converged={lst(i.converged for i in infos)} iterations={lst(i.iterations for i in infos)} operator_applications={lst(i.operator_applications for i in infos)} {sha}"


def run_variant(variant):
    problems = {}
    try:
        for case in VARIANTS[variant][1]:
            mesh = (U_CASES.get(case) or Q1_CASES[case])[0]
            P = problems.get(mesh) or problems.setdefault(mesh, problem(mesh))
            if case in U_CASES:
                print(line(variant, case, *run_u(case, P)), flush=True)
            else:
                pres, proj = run_q1(case, P)
                print(line(variant, case + "_pressure", *pres), flush=True)
                print(line(variant, case + "_projection", *proj), flush=True)
    finally:
        for P in problems.values():
            P.close()


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--variant":
        run_variant(sys.argv[2])
    else:
        for name, (env, _) in VARIANTS.items():
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--variant", name], env=dict(os.environ, **env), timeout=120, stdout=subprocess.PIPE, text=True)
            print("".join(l + "\n" for l in r.stdout.split("\n") if l.startswith(name + " ")), end="", flush=True)     # (the communicator library prints a banner of its own)
            if r.returncode != 0:
                raise SystemExit(f"variant {name}: exit status {r.returncode}; nothing further was started")
