"""Worker of the partitioned two-level tests (tests/test_partition_two_level_gpu.py): one process per rank, gloo.  Every rank builds the GLOBAL problem, takes its piece
with the coarse space (Problem.partition(rank, world, coarse=True)) and runs PREC_TWO_LEVEL on it through the HIP library; all ranks share GPU 0 and exchange through the
host-staged callback communicator.  Inputs are seeded by GLOBAL index, so the pieces hold slices of one global state.
Usage: python mr_two_level_worker.py rank world port mode mesh degree out.npz
  mode = solves (displacement, pressure and projection solves) | steps (2 fixed-stress steps, two-level everywhere) | counts (displacement solve, rel 1e-8) |
         runner (1 step with the host runner's own preconditioner choice)
  mesh = a name of test_partition_two_level_cpu.build (gmsh | refined:nx,ny[,nz] | dirichlet_3d | dirichlet_2d)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), HERE]

import poroelasticity_dealii_amd as pk  # noqa: E402
from common import REF  # noqa: E402
from test_partition_two_level_cpu import build  # noqa: E402


def seeded(n_u, n_p):
    """the global inputs of the solves (the same formulas as the single-rank tests of test_constraints_gpu.py)"""
    i, j = np.arange(n_p), np.arange(n_u)
    return {"p": REF["p_init"] * (1 + 0.3 * np.sin(0.37 * i)),
            pk.VEC_P: 10e6 * (1 + 0.05 * np.sin(0.37 * i)), pk.VEC_P_OLD: 10e6 * (1 + 0.05 * np.sin(0.2 * i)),
            pk.VEC_EPSV: -2e-6 * (1 + 0.3 * np.sin(0.5 * i)), pk.VEC_EPSV0: -2e-6 * np.ones(n_p), "u": 1e-5 * np.sin(0.05 * j)}


def proj_entries(dim):
    return [0, 2] if dim == 2 else [0, 3, 5]


def run_solves(G, P, PG, res):
    """displacement, pressure and projection solves with PREC_TWO_LEVEL; the global vectors sliced by l2g"""
    lu, lp = P.local_to_global_u, P.local_to_global_p
    S = seeded(PG.desc.n_dofs_u, PG.desc.n_dofs_p)
    res["supports"] = np.array([G.supports_preconditioner(0, pk.PREC_TWO_LEVEL), G.supports_preconditioner(1, pk.PREC_TWO_LEVEL)])
    G.set(pk.VEC_P, S["p"][lp]); G.disp_assemble_system(True)
    G.fill(pk.VEC_U, 0.0)
    rc, info = G.disp_solve(abs_tol=1e-14, rel_tol=1e-12, max_iter=500, prec=pk.PREC_TWO_LEVEL)
    res["u"] = G.get(pk.VEC_U); its = [info.iterations]; rcs = [rc]
    for k in (pk.VEC_P, pk.VEC_P_OLD, pk.VEC_EPSV, pk.VEC_EPSV0):
        G.set(k, S[k][lp])
    G.pres_assemble_residual(60.0); G.pres_assemble_jacobian(60.0)
    G.fill(pk.VEC_DP, 0.0)
    rc, info = G.pres_solve(rel_tol=1e-13, max_iter=500, prec=pk.PREC_TWO_LEVEL)
    res["dp"] = G.get(pk.VEC_DP); its.append(info.iterations); rcs.append(rc)
    dim = PG.desc.dim
    G.set(pk.VEC_U, S["u"][lu])
    G.proj_assemble_matrix(); G.proj_assemble_rhs([a * dim + a for a in range(dim)])
    for e in proj_entries(dim):
        G.fill(pk.VEC_STRAIN0 + e, 0.0)
        rc, info = G.proj_solve(e, rel_tol=1e-13, max_iter=500, prec=pk.PREC_TWO_LEVEL)
        res[f"strain{e}"] = G.get(pk.VEC_STRAIN0 + e); its.append(info.iterations); rcs.append(rc)
    res["its"] = np.array(its); res["rcs"] = np.array(rcs)


def main():
    import torch
    import torch.distributed as dist
    rank, world, port, mode, mesh, deg, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5], int(sys.argv[6]), sys.argv[7]
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)

    def allreduce(buf):
        t = torch.from_numpy(buf.copy()); dist.all_reduce(t); buf[:] = t.numpy()

    def sendrecv(send, recv, peer):
        ts, tr = torch.from_numpy(send.copy()), torch.empty(len(recv), dtype=torch.float64)
        for r in [dist.isend(ts, peer), dist.irecv(tr, peer)]:
            r.wait()
        recv[:] = tr.numpy()

    PG = build(mesh, deg)
    P = PG.partition(rank, world, coarse=True)
    res = {"l2g_u": P.local_to_global_u, "l2g_p": P.local_to_global_p, "owned": np.array([P.desc.part.n_owned_u, P.desc.part.n_owned_p])}
    if mode in ("solves", "counts"):
        G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
        G.comm_callbacks(allreduce, sendrecv)
        G.timers_reset()
        if mode == "solves":
            run_solves(G, P, PG, res)
        else:
            G.set(pk.VEC_P, REF["p_init"] * (1 + 0.3 * np.sin(0.37 * np.arange(PG.desc.n_dofs_p)))[P.local_to_global_p]); G.disp_assemble_system(True)
            rc, info = G.disp_solve(abs_tol=1e-14, rel_tol=1e-8, max_iter=2000, prec=pk.PREC_TWO_LEVEL)
            res["u"] = G.get(pk.VEC_U); res["its"] = np.array([info.iterations]); res["rcs"] = np.array([rc])
        res["coarse_allreduce_launches"] = np.array([G.timer("two_level_coarse_allreduce")[1]])
        G.close()
    else:
        kw = dict(prec=pk.PREC_TWO_LEVEL, two_level_p=True, max_it=2000) if mode == "steps" else dict(prec=-1, max_it=2000)
        R = pk.Runner(P, device=0, operator_mode=pk.OP_MATRIX_FREE, p_init=REF["p_init"], dt=REF["dt"], **kw)
        R.ctx.comm_callbacks(allreduce, sendrecv)
        R.initialize()
        rows = [np.zeros((1, 8))]
        for _ in range(2 if mode == "steps" else 1):
            rows.append(R.step()[0])
        res["trace"] = np.vstack(rows); res["u"] = R.ctx.get(pk.VEC_U); res["p"] = R.ctx.get(pk.VEC_P)
        R.close()
    np.savez(out, **res)
    P.close(); PG.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
