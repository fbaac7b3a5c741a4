"""Class-split transform passes of the block fast diagonalisation (k_fdmo_pass_vm, csrc/kernels_fdmo.hip): the single-rank octant form in fp64 on boxes whose nine
(component, direction) lines pass class_split_tables (csrc/fdm_tables.hpp).  PORO_FDMO_CLASS_SPLIT=0, read once per context build, keeps the dense passes; the
count-only timer family "fdm_u_class_split" says which form ran.

Bounds.  Against the exact block inverse: 1e-10 of max|z0|, the bound of tests/test_fdm_u_gpu.py for the fp64 block FDM; symmetry to the same 1e-10.  PCG against the
dense form: equal iteration counts, solutions to 1e-10 relative - two orders under the 1e-8 stopping reduction.  The dense form under the hook: the bits of the parent
commit (tests/golden/fdm_class_split/, produced there).

Measured on the MI355X, class-split / dense passes against the exact block inverse, in the order of BOXES: 9.2e-15 / 8.5e-15, 3.3e-14 / 5.1e-14, 5.7e-13 / 3.7e-13,
7.7e-13 / 1.9e-12, 8.8e-15 / 1.2e-14, 8.6e-14 / 9.6e-14; symmetry <= 4.3e-15.  PCG: 16 / 17 (6^3, zero / warm start) and 16 / 16 (32 x 2 x 2) iterations on both
forms under every hook combination, solutions within 1.5e-14."""
import json
import os

import numpy as np
import pytest

import poroelasticity_dealii_amd as pk
from box_reference import BoxReference
from common import BC_3D, REF, box_problem, host_material, material

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HOOK = "PORO_FDMO_CLASS_SPLIT"
FAMILY = "fdm_u_class_split"
# 1, 2, 3 and 4 class tiles in each direction, odd cell counts, classes of 16, 17, 32 and 33 entries
BOXES = [(8, 2, 2), (2, 32, 2), (2, 2, 64), (96, 2, 2), (5, 6, 7), (33, 2, 3)]
STORED = {(5, 6, 7): "dense_z_5x6x7.npy", (33, 2, 3): "dense_z_33x2x3.npy"}


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


class hooked:
    """PORO_FDMO_CLASS_SPLIT=0 (dense=True) or unset while contexts are built"""
    def __init__(self, dense):
        self.dense = dense

    def __enter__(self):
        self.old = os.environ.pop(HOOK, None)
        if self.dense:
            os.environ[HOOK] = "0"

    def __exit__(self, *exc):
        os.environ.pop(HOOK, None)
        if self.old is not None:
            os.environ[HOOK] = self.old


def assembled(P, dense=False):
    with hooked(dense):
        G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
        G.fill(pk.VEC_P, 0.0); G.disp_assemble_system(True)
        G.timers_reset()
        G.apply_preconditioner_u(pk.PREC_FDM, np.zeros(G.n_u))          # builds the preconditioner while the hook is what it is
    return G


def rhs_pair(G, mask):
    rng = np.random.default_rng(7)
    g = rng.standard_normal(G.n_u) * 1e3; g[mask] = 0.0
    g2 = rng.standard_normal(G.n_u); g2[mask] = 0.0
    return g, g2


@pytest.mark.parametrize("n", BOXES, ids=str)
def test_class_split_passes_equal_the_exact_block_inverse(n):
    P = box_problem(3, n, 2, bc=BC_3D)
    S, D = assembled(P), assembled(P, dense=True)
    try:
        R = BoxReference(P)
        g, g2 = rhs_pair(S, R.mask)
        z0 = R.block_inverse_u(g)
        zs, zd = S.apply_preconditioner_u(pk.PREC_FDM, g), D.apply_preconditioner_u(pk.PREC_FDM, g)
        es, ed = rel(zs, z0), rel(zd, z0)
        z2 = S.apply_preconditioner_u(pk.PREC_FDM, g2)
        sym = abs(g2 @ zs - g @ z2) / abs(g2 @ zs)
        print(f"class split {n} Q2: error {es:.3e} (dense passes: {ed:.3e}), symmetry {sym:.3e}, split / dense {rel(zs, zd):.3e}")
        assert S.timer(FAMILY)[1] > 0 and D.timer(FAMILY)[1] == 0
        assert np.abs(zs[R.mask]).max() == 0.0                        # constrained dofs: exact zeros
        assert es <= 1e-10, (n, es)
        assert sym <= 1e-10 and g @ zs > 0, (n, sym)
        if n in STORED:                                               # the dense form under the hook keeps the parent's bits
            assert np.array_equal(zd, np.load(os.path.join(GOLDEN, "fdm_class_split", STORED[n])))
    finally:
        S.close(); D.close(); P.close()


def test_forms_that_keep_the_dense_passes():
    """graded tensor grid, layered moduli along z, fp32 transforms: the family stays at zero, and the hook is covered above"""
    graded = pk.Problem.graded_box(3, [6, 5, 4], [10.0] * 3, 2, material(), BC_3D, [1.0, 0.5, -0.7])
    layered = box_problem(3, (4, 4, 6), 2, bc=BC_3D)
    layered.set_moduli_layers([(5.0, 1.4e10, 0.3), (10.0, 1.4e12, 0.25)])
    plain = box_problem(3, (6, 6, 6), 2, bc=BC_3D)
    try:
        for name, P, fp32 in (("graded", graded, False), ("layered", layered, False), ("fp32", plain, True), ("fp64", plain, False)):
            G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
            try:
                G.fill(pk.VEC_P, 0.0); G.disp_assemble_system(True)
                assert G.supports_preconditioner(0, pk.PREC_FDM)
                if fp32:
                    G.set_fdm_precision(pk.FDM_FP32)
                G.timers_reset()
                g = np.random.default_rng(3).standard_normal(G.n_u)
                G.apply_preconditioner_u(pk.PREC_FDM, g)
                count = G.timer(FAMILY)[1]
                print(name, "class-split applications:", count)
                assert (count > 0) == (name == "fp64"), (name, count)
            finally:
                G.close()
    finally:
        graded.close(); layered.close(); plain.close()


def solve(G, x0, **kw):
    G.set(pk.VEC_U, x0)
    rc, info = G.disp_solve(prec=pk.PREC_FDM, **kw)
    return rc, info.iterations, info.converged, G.get(pk.VEC_U)


@pytest.mark.parametrize("env", [{}, {"PORO_FDMO_SEPARATE_GZ": "1"}, {"PORO_PCG_FINAL_PREC": "1"}, {"PORO_FDMO_SEPARATE_GZ": "1", "PORO_PCG_FINAL_PREC": "1"}], ids=lambda e: "+".join(sorted(e)) or "default")
@pytest.mark.parametrize("n", [(6, 6, 6), (32, 2, 2)], ids=str)
def test_pcg_with_class_split_passes_tracks_the_dense_form(n, env):
    P = box_problem(3, n, 2)
    old = {k: os.environ.pop(k, None) for k in ("PORO_FDMO_SEPARATE_GZ", "PORO_PCG_FINAL_PREC")}
    S, D = pk.Context(P, 0, pk.OP_MATRIX_FREE), None
    try:
        with hooked(True):
            D = pk.Context(P, 0, pk.OP_MATRIX_FREE)
            for G in (S, D):
                G.set(pk.VEC_P, REF["p_init"] * (1 + 0.3 * np.sin(0.37 * np.arange(G.n_p)))); G.disp_assemble_system(True)
            D.apply_preconditioner_u(pk.PREC_FDM, np.zeros(D.n_u))
        S.timers_reset(); D.timers_reset()
        os.environ.update(env)
        bench = dict(abs_tol=1e-12, rel_tol=1e-8, max_iter=200, reduction=True)
        x0 = np.zeros(S.n_u)
        for start in ("zero", "warm"):
            rs, rd = solve(S, x0, **bench), solve(D, x0, **bench)
            e = rel(rs[3], rd[3])
            print(f"{n} from {start} {env}: {rs[1]} iterations (dense {rd[1]}), solutions differ by {e:.3e}")
            assert rs[0] == 0 and rs[:3] == rd[:3], (start, rs[:3], rd[:3])
            assert e <= 1e-10, (start, e)
            x0 = rd[3] * (1 + 1e-3 * np.cos(0.11 * np.arange(S.n_u)))          # warm start: the dense form's solution, perturbed
        # a stop at iteration 1 and a run into max_iter
        x0 = np.zeros(S.n_u)
        for kw in (dict(abs_tol=1e-12, rel_tol=0.9, max_iter=200, reduction=True), dict(abs_tol=1e-300, rel_tol=1e-30, max_iter=3, reduction=True)):
            rs, rd = solve(S, x0, **kw), solve(D, x0, **kw)
            print(f"{n} {kw}: rc {rs[0]}, {rs[1]} iterations, converged {rs[2]} (dense {rd[:3]})")
            assert rs[:3] == rd[:3], (kw, rs[:3], rd[:3])
        assert S.timer(FAMILY)[1] > 0 and D.timer(FAMILY)[1] == 0
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
        S.close()
        if D is not None:
            D.close()
        P.close()


def test_time_steps_with_class_split_passes_match_the_golden_trace():
    """3D Q2 4^3 box of tests/golden/box_traces.json, two steps through the host runner, as tests/test_fdm_fp32_gpu.py checks for its mode"""
    import oracle_py
    with open(os.path.join(GOLDEN, "box_traces.json")) as f:
        g = json.load(f)["3d_q2_4_reference"]
    P = box_problem(g["dim"], g["n"], g["degree"], mat=host_material())
    O = oracle_py.Oracle(P, hoisted=True)
    try:
        t0, _ = O.run(2, REF["p_init"], REF["dt"], max_it=5000)
        t1, G = pk.run_problem(P, 2, REF["p_init"], REF["dt"], operator_mode=pk.OP_MATRIX_FREE, max_it=5000, prec=pk.PREC_FDM)
        try:
            rows = np.array(g["rows"])
            assert t1.shape[0] == rows.shape[0] and np.array_equal(t1[:, :3], rows[:, :3]), (t1[:, :3], rows[:, :3])
            assert np.allclose(t1[:, 4], t0[:, 4], rtol=1e-8)
            rel2 = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))
            ep, eu = rel2(G.get(pk.VEC_P), O.get(pk.VEC_P)), rel2(G.get(pk.VEC_U), O.get(pk.VEC_U))
            print(f"class-split passes, 2 steps 4^3 Q2: |dp|/|p| = {ep:.2e}, |du|/|u| = {eu:.2e}, CG iterations per step {t1[1:, 6]}")
            assert ep <= 1e-9 and eu <= 1e-7, (ep, eu)
            assert G.timer(FAMILY)[1] > 0
        finally:
            G.close()
    finally:
        O.close(); P.close()
