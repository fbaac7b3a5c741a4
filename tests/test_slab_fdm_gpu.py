"""The slab-partitioned fast diagonalisation, one application at a time, against the exact inverses of the single-rank box (tests/box_reference.py): the ranks are threads
of this process (tests/slab_ranks.py, tools/rank_threads.py), every rank owns a context, and all call the hook together, each with its window of a global vector.

(A) apply_preconditioner_u(PREC_FDM) on W ranks, stitched, against BoxReference.block_inverse_u of the whole box: zero on the Dirichlet dofs, equal copies of every shared
plane (1e-13 max|z0|), 1e-10 max|z0| from the block inverse, symmetric and positive with global dots (1e-10), bitwise repeatable after another vector went through the
exchange buffers, the form asserted through the fdm_u_slab_z_stage timer; PREC_JACOBI against g / diag_A on every local row (1e-13: the assembled diagonal of the shared planes).
(B) the distributed direct solves of the Q1 systems: pres_solve and proj_solve_many with PREC_FDM against jacobian_p_inverse / mass_p_inverse of the stitched right-hand sides
(1e-10); every system must come back as solved directly (iterations == 0).  The stored right-hand sides (VEC_RESIDUAL_P, VEC_PROJ_RHS*) hold the ASSEMBLED value on a shared
plane, not a partial sum: the assembly ends with exchange_add (ctx.hip), so both copies are equal - asserted - and the stitch takes one of them.

Forms and tile counts (tests/slab_ranks.py: FDM_U_CASES; tests/test_slab_reference_cpu.py checks the arithmetic): quadrant slab form with 1 .. 8 tiles per half line - (4,3,7) on 3
ranks: 1, two-workgroup z stage; (3,2,24) on 2 and 5: 2, both-parity z pass, the last of 5 shares empty; (3,2,40) on 3 and 8: 3, the last two of 8 shares empty; (2,3,48) on 4: 4;
(3,2,72) on 3: 5; (2,2,88) on 2: 6; (2,2,104) on 3: 7; (2,2,120) on 2: 8; the 2-, 4- and 5-tile cases again with PORO_FDMO_SLAB_TWO_PARITY_WORKGROUPS; planes larger than a
chunk: (10,9,24) on 3 (2 tiles) and (9,10,12) on 4 (1 tile), whose shares end on block boundaries, and (6,5,7) on 5 (1 tile), where blocks 2, 5 and 10 lie in two shares (the second
base of the destination computation).  With 12 blocks a share is at least a block long up to 12 ranks, so the per-column division (scols < col_unit) cannot be reached by the
displacement form on the 8 contexts a case may hold; the fused Q1 form reaches it, (10,9,8) on 3 ranks in (B).  Q1 displacement (5,4,9) on 3: slab form, 1 tile.  Nodal
distributed form: (4,3,7) with PORO_FDMU_NO_OCT; (3,4,6) with the mixed Dirichlet list (different ends along a line); (2,2,130) on 2 (half line 131 > 128); 2D (6,9) Q2 on 3;
2D (2,9) Q1 on 4 (3 columns: the last rank has none).  (B): fused scalar slab form with 1, 2, 3, 5 and 8 tiles - (3,2,8) on 3, (2,3,20) on 2, (2,2,40) on 5 (one chunk: four
empty shares), (2,2,72) on 3, (2,2,120) on 4 - and (10,9,8) on 3; nodal form on (2,2,130) on 2 (131 vertices), with PORO_FDM_P_UNFUSED on (3,2,8), and in 2D on (5,9) on 3 and (2,9) on 4.

Measured on one MI355X, worst over the cases of a family, relative to max|reference| (every line of a run with -s shows its figures):
  (A) slab form, 1 .. 5 tiles (both z-stage variants)     block inverse 3.1e-13 (5 tiles)    symmetry 1.0e-14   Jacobi 7.5e-15
      slab form, 6, 7, 8 tiles                             1.4e-12, 6.2e-13, 1.0e-12          1.1e-15            1.5e-14
      planes larger than a chunk; Q1 displacement          7.9e-14 (10,9,24); 1.5e-15         5.0e-15            1.5e-15
      nodal distributed form                               2.1e-12 ((2,2,130); others <= 1.2e-14)   4.8e-15      8.3e-15
      the two copies of every shared plane: bitwise equal in every case; third application bitwise equal to the first in every case
      (the thin, long boxes are where the reference itself is 5e-13 .. 1e-12 from sparse direct solves, tests/test_slab_reference_cpu.py)
  (B) fused scalar slab form                               pressure 3.5e-13 ((2,2,72))        projection 4.3e-14 ((2,2,120))
      nodal form                                           pressure 7.5e-13 ((2,2,130))       projection 5.8e-14; 2D: 4.7e-15 / 3.2e-15
No defect found.  The tests bite (scratch builds, not committed): (i) with one eigenvalue (mode 1) of the global last-direction table scaled by 1 + 1e-6 - the slab form's and
last_global's tables of the displacement system, the fused and the nodal table of the Q1 systems - all 22 cases of (A) fail (block inverse 1.9e-9 .. 1.0e-7) and all 10 pressure
solves of (B) (6.4e-10 .. 2.2e-8; the projection's mass matrix has no stiffness term and stays exact), while tests/test_rank_threads_gpu.py passes whole and
13 of the 14 tests of tests/test_multirank_gpu.py pass; its one-rank test_rccl_data_plane_single_rank (the pressure update against the oracle at 1e-9) fails at 2.6e-9.  (ii) concerns dot
products: tests/test_slab_iterates_gpu.py."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import poroelasticity_dealii_amd as pk
import slab_ranks as sr
from box_reference import BoxReference

pytestmark = pytest.mark.gpu

DT = sr.rank_threads.REF["dt"]
P_INIT = sr.rank_threads.REF["p_init"]


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def set_env(monkeypatch, env):
    for k in ("PORO_FDMO_SLAB_TWO_PARITY_WORKGROUPS", "PORO_FDMU_NO_OCT", "PORO_FDM_P_UNFUSED"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ---- (A) ----------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(sr.FDM_U_CASES))
def test_one_application_of_the_displacement_preconditioner(monkeypatch, case):
    dim, n, deg, world, bc, env, form, nt = sr.FDM_U_CASES[case]
    set_env(monkeypatch, env)                               # (read with getenv when the tables are built: before the contexts exist)
    S = sr.Slabs(dim, n, deg, world, bc)
    P1 = sr.problem(dim, n, deg, bc=bc)
    try:
        R = BoxReference(P1)
        assert R.n_u == S.N_u
        rng = np.random.default_rng(7)
        g = rng.standard_normal(R.n_u) * 1e3; g[R.mask] = 0.0
        g2 = rng.standard_normal(R.n_u); g2[R.mask] = 0.0

        def on_rank(r, P, comm):
            G = sr.context(P, r, comm)
            try:
                assert G.supports_preconditioner(0, pk.PREC_FDM)
                G.fill(pk.VEC_P, 0.0); G.disp_assemble_system(True)
                G.timers_reset()
                gw, g2w = S.window_u(g, r), S.window_u(g2, r)
                za = G.apply_preconditioner_u(pk.PREC_FDM, gw)
                zb = G.apply_preconditioner_u(pk.PREC_FDM, g2w)
                zc = G.apply_preconditioner_u(pk.PREC_FDM, gw)
                stages = G.timer("fdm_u_slab_z_stage")[1]
                return dict(z=za, z2=zb, z_again=zc, stages=stages, jacobi=G.apply_preconditioner_u(pk.PREC_JACOBI, gw))
            finally:
                G.close()
        out = S.run(on_rank)
        z0 = R.block_inverse_u(g)
        scale = float(np.abs(z0).max())
        # 6. the form that ran
        for r, o in enumerate(out):
            assert (o["stages"] >= 1) if form == "slab" else (o["stages"] == 0), (case, r, o["stages"])
        # 2. the two copies of every shared plane
        shared = max(float(np.abs(a - b).max()) for key in ("z", "z2") for a, b in sr.shared_copies([o[key] for o in out], S.plane_u))
        z, z2 = S.stitch_u([o["z"] for o in out]), S.stitch_u([o["z2"] for o in out])
        e = float(np.abs(z - z0).max() / scale)
        sym = abs(g2 @ z - g @ z2) / abs(g2 @ z)
        d = R.diag_A()
        ej = max(float(np.abs(o["jacobi"] - S.window_u(g, r) / S.window_u(d, r)).max() / np.abs(g / d).max()) for r, o in enumerate(out))
        print(f"slab fdm {case}: form {form} tiles {nt} layers {S.layers}: block inverse {e:.2e} shared planes {shared / scale:.2e} symmetry {sym:.2e} jacobi {ej:.2e}", flush=True)
        assert np.abs(z[R.mask]).max() == 0.0 and np.abs(z2[R.mask]).max() == 0.0                                 # 1.
        assert shared <= 1e-13 * scale, (case, shared / scale)                                                       # 2. (z2 is of the size of z / 1e3: the same absolute bound asks more of it)
        assert e <= 1e-10, (case, e)                                                                                 # 3.
        assert sym <= 1e-10 and g @ z > 0 and g2 @ z2 > 0, (case, sym)                                              # 4.
        for r, o in enumerate(out):                                                                                  # 5.
            assert np.array_equal(o["z_again"], o["z"]), (case, r, float(np.abs(o["z_again"] - o["z"]).max()))
        assert ej <= 1e-13, (case, ej)                                                                               # 7.
    finally:
        S.close(); P1.close()


# ---- (B) ----------------------------------------------------------------------------------------------------------------------------------------------------------------
UNFUSED = {"PORO_FDM_P_UNFUSED": "1"}
# name -> (dim, cells, ranks, environment)
Q1_CASES = {"fused_nt1_3x2x8_w3": (3, (3, 2, 8), 3, {}), "fused_nt2_2x3x20_w2": (3, (2, 3, 20), 2, {}), "fused_nt3_2x2x40_w5": (3, (2, 2, 40), 5, {}), "fused_nt5_2x2x72_w3": (3, (2, 2, 72), 3, {}),
            "fused_nt8_2x2x120_w4": (3, (2, 2, 120), 4, {}), "fused_plane_10x9x8_w3": (3, (10, 9, 8), 3, {}), "nodal_long_2x2x130_w2": (3, (2, 2, 130), 2, {}),
            "nodal_unfused_3x2x8_w3": (3, (3, 2, 8), 3, UNFUSED), "nodal_2d_5x9_w3": (2, (5, 9), 3, {}), "nodal_2d_2x9_w4": (2, (2, 9), 4, {})}


def test_the_fused_q1_cases_visit_both_destination_computations():
    lay = {k: sr.slab_shares(v[1], 1, v[2], scalar=True) for k, v in Q1_CASES.items() if k.startswith("fused")}
    assert sorted(L["nt"] for L in lay.values()) == [1, 1, 2, 3, 5, 8]
    assert not lay["fused_plane_10x9x8_w3"]["share_at_least_a_block"] and lay["fused_nt1_3x2x8_w3"]["share_at_least_a_block"]
    assert lay["fused_nt3_2x2x40_w5"]["my_chunks"] == [1, 0, 0, 0, 0]
    assert 130 + 1 > 16 * sr.max_tiles()                    # the long box: 131 vertices, beyond the fused kernels
    assert sr.nodal_columns((2, 9), 1, 2, 4, q1=True) == [1, 1, 1, 0]


@pytest.mark.parametrize("case", list(Q1_CASES))
def test_distributed_q1_direct_solves_are_the_exact_inverses(monkeypatch, case):
    dim, n, world, env = Q1_CASES[case]
    set_env(monkeypatch, env)
    S = sr.Slabs(dim, n, 1, world)
    P1 = sr.problem(dim, n, 1)
    try:
        R = BoxReference(P1)
        i, j = np.arange(R.n_p), np.arange(R.n_u)
        vals = {pk.VEC_P: P_INIT * (1 + 0.3 * np.sin(0.37 * i)), pk.VEC_P_OLD: P_INIT * (1 + 0.1 * np.cos(0.21 * i)), pk.VEC_EPSV: 1e-6 * np.sin(0.13 * i), pk.VEC_EPSV0: np.zeros(R.n_p)}
        u = 1e-5 * np.sin(0.37 * j) + 1e-6 * np.cos(0.05 * j)
        ent = list(range(dim * (dim + 1) // 2))
        full = [a * dim + b for a in range(dim) for b in range(a, dim)]

        def on_rank(r, P, comm):
            G = sr.context(P, r, comm)
            try:
                assert G.supports_preconditioner(1, pk.PREC_FDM)
                for k, v in vals.items():
                    G.set(k, S.window_p(v, r))
                G.pres_assemble_residual(DT); G.pres_assemble_jacobian(DT); G.fill(pk.VEC_DP, 0.0)
                rc, info = G.pres_solve(prec=pk.PREC_FDM)
                o = dict(rc=rc, its=info.iterations, rhs=G.get(pk.VEC_RESIDUAL_P), dp=G.get(pk.VEC_DP))
                G.set(pk.VEC_U, S.window_u(u, r)); G.proj_assemble_matrix(); G.proj_assemble_rhs(full)
                rc, infos = 0, []
                for first in range(0, len(ent), 3):           # (the direct solve takes up to three systems per call; more are handed to proj_solve one by one, which iterates)
                    rc_, infos_ = G.proj_solve_many(ent[first: first + 3], prec=pk.PREC_FDM)
                    rc, infos = max(rc, rc_), infos + infos_
                o.update(rc_proj=rc, its_proj=[f.iterations for f in infos], proj_rhs=[G.get(pk.VEC_PROJ_RHS0 + e) for e in ent], strain=[G.get(pk.VEC_STRAIN0 + e) for e in ent])
                return o
            finally:
                G.close()
        out = S.run(on_rank)
        assert all(o["rc"] == 0 and o["its"] == 0 and o["rc_proj"] == 0 and o["its_proj"] == [0] * len(ent) for o in out), [(o["rc"], o["its"], o["rc_proj"], o["its_proj"]) for o in out]

        def stitched(parts, what, check_copies):
            scale = max(float(np.abs(p).max()) for p in parts)
            worst = max((float(np.abs(a - b).max()) for a, b in sr.shared_copies(parts, S.plane_p)), default=0.0)
            assert worst <= check_copies * scale, (case, what, worst / scale)
            return S.stitch_p(parts)
        r_glob = stitched([o["rhs"] for o in out], "residual", 1e-13)                      # assembled on the shared planes: both copies hold the sum
        e_p = rel(stitched([o["dp"] for o in out], "dp", 1e-13), R.jacobian_p_inverse(r_glob, DT))
        e_s = 0.0
        for k, e_ in enumerate(ent):
            b = stitched([o["proj_rhs"][k] for o in out], f"projection rhs {e_}", 1e-13)
            e_s = max(e_s, rel(stitched([o["strain"][k] for o in out], f"strain {e_}", 1e-13), R.mass_p_inverse(b)))
        print(f"slab q1 {case}: layers {S.layers}: pressure {e_p:.2e} projection {e_s:.2e}", flush=True)
        assert e_p <= 1e-10, (case, "pressure", e_p)
        assert e_s <= 1e-10, (case, "projection", e_s)
    finally:
        S.close(); P1.close()
