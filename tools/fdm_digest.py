"""SHA-256 digests of fast-diagonalisation results on the smallest shapes that reach every table uploader and every form decision of the displacement set-up, plus a
pressure and a projection solve of the 9 x 5 x 2 Q1 box.  Two commits whose outputs are equal line for line compute the same bits there.

    python tools/fdm_digest.py                    every variant, one fresh child process each (the switches are read once per process), stopping at the first failure
    python tools/fdm_digest.py --variant NAME     the cases of one variant in this process, under whatever environment the caller set"""
import hashlib, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path[:0] = [ROOT]
import numpy as np
import poroelasticity_dealii_amd as pk
import bench

BC_2D, BC_3D = bench.BC_3D[:4], bench.BC_3D
# (name, cells, degree, Dirichlet list, grading): see the table in tests/test_fdm_table_paths_gpu.py
OCT_Q2 = ("oct_q2", (3, 4, 5), 2, BC_3D, None)
SHAPES = [OCT_Q2, ("oct_q1", (3, 4, 5), 1, BC_3D, None),
          ("nodal_full_x_split_yz", (3, 4, 5), 2, [(0, 0, 0.0)] + BC_3D[2:], None),
          ("nodal_full", (3, 4, 5), 2, [(0, 0, 0.0), (2, 1, 0.0), (4, 2, 0.0)], None),
          ("planar_split", (5, 7), 2, BC_2D, None),
          ("planar_unsplit", (5, 7), 2, [(2, 1, 0.0), (1, 0, -1e-5)], None),
          ("graded_same_ends", (4, 3, 5), 2, BC_3D, (1.0, 0.5, -0.7))]
NO_OCT = {"PORO_FDMU_NO_OCT": "1"}
VARIANTS = {"default": ({}, SHAPES + ["q1"]),
            "no_oct": (NO_OCT, [OCT_Q2, ("blocked_split_163", (81, 2), 2, BC_2D, None)]),
            "no_oct_lds_form": (dict(NO_OCT, PORO_FDMU_LDS_FORM="1"), [OCT_Q2]),
            "no_oct_no_split": (dict(NO_OCT, PORO_FDMU_NO_SPLIT="1"), [OCT_Q2]),
            "no_oct_single": (dict(NO_OCT, PORO_FDMU_SINGLE="1"), [OCT_Q2]),
            "p_unfused": ({"PORO_FDM_P_UNFUSED": "1"}, ["q1"])}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def block_fdm(variant, name, n, deg, bc, grading):
    dim = len(n)
    if grading is None:
        P = pk.Problem.box(dim, list(n), [10.0] * dim, deg, bench.material(), bc)
    else:
        P = pk.Problem.graded_box(dim, list(n), [10.0] * dim, deg, bench.material(), bc, list(grading))
    G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    d = P.desc
    fixed = np.ctypeslib.as_array(d.dirichlet_dof, shape=(d.n_dirichlet,)).copy()
    G.fill(pk.VEC_P, 0.0); G.disp_assemble_system(True)
    g = np.random.default_rng(7).standard_normal(G.n_u) * 1e3; g[fixed] = 0.0
    print(variant, name, sha(G.apply_preconditioner_u(pk.PREC_FDM, g)), flush=True)
    G.close(); P.close()


def q1_solves(variant):
    P = pk.Problem.box(3, [9, 5, 2], [10.0] * 3, 1, bench.material(), BC_3D)
    G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    p0, dt, i = bench.INPUT["p_init"], bench.INPUT["dt"], np.arange(G.n_p)
    G.set(pk.VEC_P, p0 * (1 + 0.3 * np.sin(0.37 * i))); G.set(pk.VEC_P_OLD, p0 * (1 + 0.1 * np.cos(0.21 * i)))
    G.set(pk.VEC_EPSV, 1e-6 * np.sin(0.13 * i)); G.fill(pk.VEC_EPSV0, 0.0)
    G.pres_assemble_residual(dt); G.pres_assemble_jacobian(dt); G.fill(pk.VEC_DP, 0.0)
    rc, _ = G.pres_solve(prec=pk.PREC_FDM)
    assert rc == 0
    print(variant, "q1_pressure", sha(G.get(pk.VEC_DP)), flush=True)
    j = np.arange(G.n_u)
    G.set(pk.VEC_U, 1e-5 * np.sin(0.37 * j) + 1e-6 * np.cos(0.05 * j))
    G.proj_assemble_matrix(); G.proj_assemble_rhs([a * 3 + b for a in range(3) for b in range(a, 3)])
    rc, _ = G.proj_solve_many(list(range(6)), prec=pk.PREC_FDM)
    assert rc == 0
    print(variant, "q1_projection", sha(np.concatenate([G.get(pk.VEC_STRAIN0 + e) for e in range(6)])), flush=True)
    G.close(); P.close()


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--variant":
        for case in VARIANTS[sys.argv[2]][1]:
            q1_solves(sys.argv[2]) if case == "q1" else block_fdm(sys.argv[2], *case)
    else:
        for name, (env, _) in VARIANTS.items():
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--variant", name], env=dict(os.environ, **env), timeout=120)
            if r.returncode != 0:
                raise SystemExit(f"variant {name}: exit status {r.returncode}; nothing further was started")
