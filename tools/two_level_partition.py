"""PORO_PREC_TWO_LEVEL on the pieces of a general partition (Problem.partition(..., coarse=True)): CG iteration counts and communication volume on locally refined 3D Q2
boxes, next to Chebyshev (the best partitioned displacement preconditioner without a coarse space) and Jacobi.  N <= 4 rank processes share one GPU and exchange
through gloo (the host-staged callback communicator), so only clock-independent facts are recorded: iterations, all-reduces per iteration (counted launches of the
"allreduce" and "two_level_coarse_allreduce" timer families, initial residual and set-up included) and the bytes of one coarse all-reduce.
Usage: python tools/two_level_partition.py [--sizes 8,16,32] [--ranks 1,2,4] [--out profiles/two_level_partition.json] [--ab AB.json]
       (--ab: a file holding the "single_rank_ab" record to store alongside)"""
import argparse, ctypes, json, os, socket, subprocess, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path[:0] = [ROOT]
import poroelasticity_dealii_amd as pk
import bench

JACOBI_MAX_N = 16


def problem(n):
    return pk.Problem.refined_box(3, [n] * 3, [10.0] * 3, 2, bench.material(), bench.BC_3D, [n // 4] * 3, [3 * n // 4] * 3)


def counts(G, its):
    ar = G.timer("allreduce")[1]; co = G.timer("two_level_coarse_allreduce")[1]
    return {"cg_iterations": int(its), "allreduces": int(ar + co), "coarse_allreduces": int(co),
            "allreduces_per_iteration": round((ar + co) / max(its, 1), 3)}


def worker(rank, world, port, n, out):
    comm = None
    if world > 1:
        import torch
        import torch.distributed as dist
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)

        def allreduce(buf):
            t = torch.from_numpy(buf.copy()); dist.all_reduce(t); buf[:] = t.numpy()

        def sendrecv(send, recv, peer):
            ts, tr = torch.from_numpy(send.copy()), torch.empty(len(recv), dtype=torch.float64)
            for r in [dist.isend(ts, peer), dist.irecv(tr, peer)]:
                r.wait()
            recv[:] = tr.numpy()
        comm = (allreduce, sendrecv)
    PG = problem(n)
    P = PG.partition(rank, world, coarse=True) if world > 1 else PG
    lp = P.local_to_global_p if world > 1 else np.arange(PG.desc.n_dofs_p)
    G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    if comm:
        G.comm_callbacks(*comm)
    box = ctypes.cast(P.desc.coarse.box_problem, ctypes.POINTER(pk.Desc)).contents
    i_p = np.arange(PG.desc.n_dofs_p)
    rec = {"coarse_cells": n, "ranks": world, "n_dofs_u": int(PG.desc.n_dofs_u), "n_dofs_p": int(PG.desc.n_dofs_p),
           "coarse_allreduce_bytes_u": 8 * int(box.n_dofs_u), "coarse_allreduce_bytes_p": 8 * int(box.n_dofs_p), "displacement": {}, "pressure": {}}
    G.set(pk.VEC_P, (bench.INPUT["p_init"] * (1 + 0.3 * np.sin(0.37 * i_p)))[lp]); G.disp_assemble_system(True)
    for name, prec, cap in (("two_level", pk.PREC_TWO_LEVEL, 2000), ("chebyshev", pk.PREC_CHEBYSHEV, 20000), ("jacobi", pk.PREC_JACOBI, 100000)):
        if name == "jacobi" and n > JACOBI_MAX_N:
            continue
        G.fill(pk.VEC_U, 0.0); G.timers_reset()
        rc, info = G.disp_solve(abs_tol=1e-14, rel_tol=1e-8, max_iter=cap, prec=prec)
        rec["displacement"][name] = dict(counts(G, info.iterations), converged=rc == 0)
    vals = {pk.VEC_P: 10e6 * (1 + 0.05 * np.sin(0.37 * i_p)), pk.VEC_P_OLD: 10e6 * (1 + 0.05 * np.sin(0.2 * i_p)),
            pk.VEC_EPSV: -2e-6 * (1 + 0.3 * np.sin(0.5 * i_p)), pk.VEC_EPSV0: -2e-6 * np.ones(len(i_p))}
    for k, v in vals.items():
        G.set(k, v[lp])
    G.pres_assemble_residual(60.0); G.pres_assemble_jacobian(60.0)
    for name, prec, cap in (("two_level", pk.PREC_TWO_LEVEL, 2000), ("jacobi", pk.PREC_JACOBI, 100000)):
        G.fill(pk.VEC_DP, 0.0); G.timers_reset()
        rc, info = G.pres_solve(rel_tol=1e-8, max_iter=cap, prec=prec)
        rec["pressure"][name] = dict(counts(G, info.iterations), converged=rc == 0)
    G.close()
    if P is not PG:
        P.close()
    PG.close()
    if rank == 0:
        with open(out, "w") as f:
            json.dump(rec, f)
    if world > 1:
        dist.barrier(); dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8,16,32"); ap.add_argument("--ranks", default="1,2,4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "two_level_partition.json")); ap.add_argument("--ab", default=None)
    ap.add_argument("--worker", nargs=5, default=None)
    a = ap.parse_args()
    if a.worker:
        r, w, port, n, out = a.worker
        worker(int(r), int(w), int(port), int(n), out); return
    cases = []
    for n in [int(v) for v in a.sizes.split(",")]:
        for world in [int(v) for v in a.ranks.split(",")]:
            assert 1 <= world <= 4
            s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
            tmp = f"{a.out}.part"
            procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", str(r), str(world), str(port), str(n), tmp], env=dict(os.environ, OMP_NUM_THREADS="1"))
                     for r in range(world)]
            if any(p.wait(timeout=900) != 0 for p in procs):
                sys.exit(f"a rank failed: n = {n}, {world} ranks")
            with open(tmp) as f:
                cases.append(json.load(f))
            os.remove(tmp)
            print(json.dumps(cases[-1]), flush=True)
    doc = {"mesh": "n^3 box, cells [n/4, 3n/4)^3 refined once (hanging nodes), Q2/Q1, bench.py material and boundary conditions",
           "setting": "pieces of Problem.partition(rank, ranks, coarse=True), ranks sharing one GPU through gloo (callback communicator); 1 rank = the unpartitioned problem",
           "solves": "displacement abs 1e-14 / rel 1e-8; pressure Jacobian (dt = 60 s) rel 1e-8; zero initial guess; jacobi displacement only for n <= %d" % JACOBI_MAX_N,
           "allreduces": "launches of the all-reduce timer families during one solve (scalar all-reduces incl. set-up + one coarse all-reduce per preconditioner application)",
           "coarse_allreduce_bytes": "8 * dim * box displacement nodes (displacement), 8 * box vertices (pressure and projection) per preconditioner application",
           "cases": cases}
    if a.ab:
        with open(a.ab) as f:
            doc["single_rank_ab"] = json.load(f)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
