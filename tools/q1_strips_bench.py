"""times the three scalar fast-diagonalisation passes (timer family precondition_p_fdm) in the block-per-workgroup form and in the strip form, for 1 right-hand side
(the direct pressure solve) and 3 (the batched projection solve), on boxes of N^3 vertices: the measurement behind kFdmoStripFill (common.hpp).
usage: q1_strips_bench.py [N ...]      (default 24 48 72 120; REPS=50)
The form is forced through PORO_FDMO_SCALAR_STRIPS (0: block form; a huge factor: strips whatever the launch size), read when a context builds its tables."""
import json, os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, os.path.join(R, "oracle"), os.path.join(R, "tests")]
import numpy as np
import poroelasticity_dealii_amd as pk
from common import material

REPS = int(os.environ.get("REPS", "50"))
DT = 60.0


def measure(nv, factor):
    os.environ["PORO_FDMO_SCALAR_STRIPS"] = factor
    n = [nv - 1] * 3
    P = pk.Problem.box(3, n, [float(m) for m in n], 1, material(), [(2 * d, d, 0.0) for d in range(3)])
    G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    out = {}
    try:
        G.timers_enable(True)
        b = np.random.default_rng(7).standard_normal(G.n_p)
        G.pres_assemble_jacobian(DT)
        G.set(pk.VEC_U, 1e-5 * np.sin(0.05 * np.arange(G.n_u))); G.proj_assemble_matrix(); G.proj_assemble_rhs([0, 4, 8])
        for nb in (1, 3):
            for rep in range(REPS + 5):
                if rep == 5:
                    G.timers_reset()                       # (the first calls build tables and warm caches)
                if nb == 1:
                    G.set(pk.VEC_RESIDUAL_P, b); G.fill(pk.VEC_DP, 0.0)
                    rc, info = G.pres_solve(rel_tol=1e-8, prec=pk.PREC_FDM)
                    assert rc == 0 and info.iterations == 0
                else:
                    rc, infos = G.proj_solve_many([0, 3, 5], rel_tol=1e-8, prec=pk.PREC_FDM)
                    assert rc == 0 and all(i.iterations == 0 for i in infos)
            sec, cnt = G.timer("precondition_p_fdm")
            out[f"rhs{nb}_us"] = round(1e6 * sec / max(cnt, 1), 2)
            out[f"rhs{nb}_strip_launches_per_call"] = G.timer("fdm_q1_strip_launches")[1] / max(cnt, 1)
    finally:
        G.close(); P.close()
    return out


if __name__ == "__main__":
    sizes = [int(v) for v in sys.argv[1:]] or [24, 48, 72, 120]
    for nv in sizes:
        res = {"vertices_per_side": nv, "tiles": (nv + 15) // 16, "block": measure(nv, "0"), "strips": measure(nv, "1e9")}
        print(json.dumps(res), flush=True)
