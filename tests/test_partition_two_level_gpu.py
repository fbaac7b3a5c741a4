"""PREC_TWO_LEVEL on the pieces of a general partition: 2-4 ranks share GPU 0 over gloo (tests/mr_two_level_worker.py), each piece carrying the coarse space
(Problem.partition(..., coarse=True)); the restriction runs over the owned rows, one all-reduce of the coarse vector per application, the coarse solve replicated.
Against the oracle's Jacobi-CG and the single-rank two-level solve on the global problem."""
import os
import subprocess
import sys

import numpy as np
import pytest

import poroelasticity_dealii_amd as pk
import oracle_py
from common import REF
from mr_two_level_worker import proj_entries, run_solves, seeded
from test_multirank_cpu import HERE, free_port
from test_partition_general_cpu import assemble_global
from test_partition_two_level_cpu import build

pytestmark = pytest.mark.gpu


def rel2(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def run_ranks(tmp_path, world, mode, mesh, deg):
    assert world <= 4
    port = free_port()
    outs = [str(tmp_path / f"{mode}{r}.npz") for r in range(world)]
    env = dict(os.environ, OMP_NUM_THREADS="1")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "mr_two_level_worker.py"), str(r), str(world), str(port), mode, mesh, str(deg), outs[r]], env=env)
             for r in range(world)]
    for p in procs:
        assert p.wait(timeout=900) == 0
    return [np.load(o) for o in outs]


class _Whole:
    """the global problem seen as its own single piece (identity local -> global maps)"""
    def __init__(self, P):
        self.local_to_global_u = np.arange(P.desc.n_dofs_u); self.local_to_global_p = np.arange(P.desc.n_dofs_p)


SOLVE_CASES = [(2, "refined:4,4,4", 2), (3, "refined:8,8,8", 2), (4, "refined:8,8,8", 1), (3, "refined:6,5", 1), (2, "refined:6,5", 2), (3, "gmsh", 2), (2, "gmsh", 1),
               (2, "dirichlet_2d", 1)]


@pytest.mark.parametrize("world,mesh,deg", SOLVE_CASES)
def test_partitioned_two_level_solves(tmp_path, world, mesh, deg):
    """displacement (abs 1e-14, rel 1e-12), pressure and projection (rel 1e-13) solves with PREC_TWO_LEVEL on the pieces: within 1e-9 of the oracle's Jacobi-CG, every
    shared copy bitwise equal, iteration counts within one of the single-rank two-level solve"""
    R = run_ranks(tmp_path, world, "solves", mesh, deg)
    PG = build(mesh, deg)
    O = oracle_py.Oracle(PG, hoisted=True)
    G = pk.Context(PG, 0, pk.OP_MATRIX_FREE)
    try:
        nu, n_p, dim = PG.desc.n_dofs_u, PG.desc.n_dofs_p, PG.desc.dim
        single = {}
        run_solves(G, _Whole(PG), PG, single)
        S = seeded(nu, n_p)
        O.set(pk.VEC_P, S["p"]); O.disp_assemble_system(True)
        assert O.disp_solve(abs_tol=1e-14, rel_tol=1e-12, max_iter=50000)[0] == 0
        u_ref = O.get(pk.VEC_U)                 # (the projection right-hand sides below overwrite VEC_U)
        for k in (pk.VEC_P, pk.VEC_P_OLD, pk.VEC_EPSV, pk.VEC_EPSV0):
            O.set(k, S[k])
        O.pres_assemble_residual(60.0); O.pres_assemble_jacobian(60.0)
        assert O.pres_solve(rel_tol=1e-13, max_iter=5000)[0] == 0
        O.set(pk.VEC_U, S["u"]); O.proj_assemble_matrix(); O.proj_assemble_rhs([a * dim + a for a in range(dim)])
        for e in proj_entries(dim):
            assert O.proj_solve(e, rel_tol=1e-13, max_iter=5000)[0] == 0
        print(f"{mesh} Q{deg} on {world} ranks: two-level iterations per solve (u, p, projections) pieces {R[0]['its'].tolist()} single rank {single['its'].tolist()}, "
              f"differences {(R[0]['its'] - single['its']).tolist()}")
        for r in R:
            assert r["supports"].all() and np.all(r["rcs"] == 0)
            assert np.array_equal(r["its"], R[0]["its"])
            assert np.all(np.abs(r["its"] - single["its"]) <= 1), (r["its"], single["its"])
            assert r["coarse_allreduce_launches"][0] > 0
        assert sum(int(r["owned"][0]) for r in R) == nu and sum(int(r["owned"][1]) for r in R) == n_p
        assert rel2(assemble_global(R, "u", "l2g_u", nu), u_ref) <= 1e-9
        assert rel2(single["u"], u_ref) <= 1e-9
        assert rel2(assemble_global(R, "dp", "l2g_p", n_p), O.get(pk.VEC_DP)) <= 1e-9
        for e in proj_entries(dim):
            assert rel2(assemble_global(R, f"strain{e}", "l2g_p", n_p), O.get(pk.VEC_STRAIN0 + e)) <= 1e-9
    finally:
        G.close(); O.close(); PG.close()


@pytest.mark.parametrize("world", [2, 3])
def test_partitioned_two_level_time_steps_track_the_oracle(tmp_path, world):
    """the refined mesh of test_time_steps_with_the_two_level_solvers_track_the_oracle (its block touches the bottom Dirichlet face; on 3 ranks its pieces need the
    per-node ghosting), 2 fixed-stress steps with PREC_TWO_LEVEL on all three systems against the oracle's Jacobi run"""
    R = run_ranks(tmp_path, world, "steps", "dirichlet_3d", 2)
    PG = build("dirichlet_3d", 2)
    O = oracle_py.Oracle(PG, hoisted=True)
    try:
        t0, _ = O.run(2, REF["p_init"], REF["dt"], max_it=20000, prec=oracle_py.PREC_JACOBI)
        for r in R:
            assert np.array_equal(r["trace"][1:, :3], t0[1:, :3])
        u = assemble_global(R, "u", "l2g_u", PG.desc.n_dofs_u); p = assemble_global(R, "p", "l2g_p", PG.desc.n_dofs_p)
        assert rel2(u, O.get(pk.VEC_U)) <= 1e-7
        assert np.abs(p - O.get(pk.VEC_P)).max() <= 1e-9 * np.abs(O.get(pk.VEC_P)).max()
    finally:
        O.close(); PG.close()


def test_partitioned_two_level_counts_do_not_grow_with_refinement(tmp_path):
    """refined 3D Q2 boxes n = 4, 8, 16 on 3 ranks (rel 1e-8): at most 1.3x more iterations per level, each count within one of the single-rank count"""
    pieces, single = [], []
    for n in (4, 8, 16):
        mesh = f"refined:{n},{n},{n}"
        R = run_ranks(tmp_path, 3, "counts", mesh, 2)
        assert all(r["rcs"][0] == 0 and r["its"][0] == R[0]["its"][0] for r in R)
        pieces.append(int(R[0]["its"][0]))
        PG = build(mesh, 2); G = pk.Context(PG, 0, pk.OP_MATRIX_FREE)
        try:
            G.set(pk.VEC_P, REF["p_init"] * (1 + 0.3 * np.sin(0.37 * np.arange(G.n_p)))); G.disp_assemble_system(True)
            rc, info = G.disp_solve(abs_tol=1e-14, rel_tol=1e-8, max_iter=2000, prec=pk.PREC_TWO_LEVEL)
            assert rc == 0
            single.append(info.iterations)
        finally:
            G.close(); PG.close()
    print("two-level CG iterations, 3 ranks:", pieces, "single rank:", single, "differences:", [a - b for a, b in zip(pieces, single)])
    assert pieces[1] <= 1.3 * pieces[0] and pieces[2] <= 1.3 * pieces[1], pieces
    assert all(abs(a - b) <= 1 for a, b in zip(pieces, single)), (pieces, single)


def test_host_runner_chooses_like_a_single_rank(tmp_path):
    """refined:16,16,16 Q2 (9097 pressure dofs in all, fewer than 4096 on every one of 3 pieces): Runner(prec=-1) picks the two-level pressure preconditioner on the
    pieces as on one rank, from the global dof count"""
    R = run_ranks(tmp_path, 3, "runner", "refined:16,16,16", 2)
    PG = build("refined:16,16,16", 2)
    try:
        assert PG.desc.n_dofs_p >= 4096 and all(len(r["l2g_p"]) < 4096 for r in R)
        S = pk.Runner(PG, device=0, operator_mode=pk.OP_MATRIX_FREE, p_init=REF["p_init"], dt=REF["dt"], prec=-1, max_it=2000)
        try:
            S.initialize()
            t1 = S.step()[0]
        finally:
            S.close()
        for r in R:
            tr = r["trace"][1:]
            print("pieces u-CG", tr[:, 6].tolist(), "p-CG", tr[:, 7].tolist(), "single rank u-CG", t1[:, 6].tolist(), "p-CG", t1[:, 7].tolist())
            assert np.array_equal(tr[:, :3], t1[:, :3])
            assert np.all(np.abs(tr[:, 6] - t1[:, 6]) <= 1)
            assert np.all(np.abs(tr[:, 7] - t1[:, 7]) <= t1[:, 2])
    finally:
        PG.close()


def test_two_level_coarse_allreduce_through_rccl(monkeypatch):
    """the partitioned code path on one rank with a 1-rank RCCL communicator (as test_multirank_gpu.test_rccl_data_plane_single_rank for boxes) on refined:8,8,8 Q2:
    the coarse all-reduce goes through ncclAllReduce; same solution as the oracle, iterations within one of the plain single-rank solve"""
    PG = build("refined:8,8,8", 2)
    O = oracle_py.Oracle(PG, hoisted=True)
    p = REF["p_init"] * (1 + 0.3 * np.sin(0.37 * np.arange(PG.desc.n_dofs_p)))
    plain = pk.Context(PG, 0, pk.OP_MATRIX_FREE)
    G = None
    try:
        plain.set(pk.VEC_P, p); plain.disp_assemble_system(True)
        rc0, info0 = plain.disp_solve(abs_tol=1e-14, rel_tol=1e-12, max_iter=500, prec=pk.PREC_TWO_LEVEL)
        assert rc0 == 0
        O.set(pk.VEC_P, p); O.disp_assemble_system(True)
        assert O.disp_solve(abs_tol=1e-14, rel_tol=1e-12, max_iter=50000)[0] == 0
        monkeypatch.setenv("PORO_FORCE_PARTITIONED_PATH", "1")
        G = pk.Context(PG, 0, pk.OP_MATRIX_FREE)
        G.comm_rccl(pk.rccl_unique_id())
        G.timers_reset()
        G.set(pk.VEC_P, p); G.disp_assemble_system(True)
        assert G.supports_preconditioner(0, pk.PREC_TWO_LEVEL)
        rc, info = G.disp_solve(abs_tol=1e-14, rel_tol=1e-12, max_iter=500, prec=pk.PREC_TWO_LEVEL)
        launches = G.timer("two_level_coarse_allreduce")[1]
        print("RCCL path:", info.iterations, "iterations, plain single rank:", info0.iterations, "coarse all-reduces:", launches)
        assert rc == 0 and rel2(G.get(pk.VEC_U), O.get(pk.VEC_U)) <= 1e-9
        assert abs(info.iterations - info0.iterations) <= 1
        assert launches > 0
    finally:
        if G is not None:
            G.close()
        plain.close(); O.close(); PG.close()
