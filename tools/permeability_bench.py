"""Per-cell permeability on the MI355X: what the variable-coefficient kernels and the line-solve form of PREC_FDM cost next to their constant-coefficient
counterparts, and what the layer-mean preconditioner saves against Jacobi.  Writes profiles/permeability_layered.json.

    python tools/permeability_bench.py [--cells 72] [--runs 5] [--out profiles/permeability_layered.json]

Protocol (as the project's other profiles): every figure is the median of `runs` runs, the variants alternating inside each run, with max - min beside it.
Kernel times are HIP-event times per launch from the context's timers (poro_timers_get), solve times the wall time poro_pres_solve reports.
Material: biot_M = 1, k / mu = 1, dt = 1 on cells of edge 1 (a M and K_kappa of comparable size), the setting of tests/test_permeability_gpu.py."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import poroelasticity_dealii_amd as pk  # noqa: E402


def material():
    m = pk.read_input(os.path.join(ROOT, "tests", "golden", "input.data")).material
    m.biot_M, m.k_over_mu, m.flow_rate = 1.0, 1.0, 0.0
    return m


def layer_values(n):
    return 10.0 ** (-3 + 3 * ((7 * np.arange(n)) % 5) / 4)


def general_field(n):
    k, j, i = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    return (layer_values(n)[k] * (1 + 0.5 * np.sin(1.7 * i + 2.3 * j + 0.9 * k))).ravel()


def per_launch(G, name):
    s, n = G.timer(name)
    return 1e6 * s / n if n else None


def stats(v):
    v = [x for x in v if x is not None]
    return {"median": float(np.median(v)), "max_minus_min": float(max(v) - min(v)), "runs": [float(x) for x in v]} if v else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=72)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "permeability_layered.json"))
    a = ap.parse_args()
    n = a.cells
    P = pk.Problem.box(3, [n] * 3, [float(n)] * 3, 1, material(), [(0, 0, 0.0), (2, 1, 0.0), (4, 2, 0.0)])
    fields = {"constant": None, "layered": np.repeat(layer_values(n), n * n), "general": general_field(n),
              "caprock": np.repeat(np.where(np.arange(n) >= n - n // 6, 1e-3, 1.0), n * n)}
    ctx = {}
    for name, f in fields.items():
        G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
        if f is not None:
            G.set_cell_permeability(f)
        G.pres_assemble_jacobian(1.0)
        ctx[name] = G
    rng = np.random.default_rng(1)
    b = rng.standard_normal(ctx["constant"].n_p)
    state = {v: rng.standard_normal(b.size) for v in (pk.VEC_P, pk.VEC_P_OLD, pk.VEC_EPSV, pk.VEC_EPSV0)}
    for G in ctx.values():
        for v, x in state.items():
            G.set(v, x)

    def solve(G, prec, rel_tol):
        G.set(pk.VEC_RESIDUAL_P, b); G.fill(pk.VEC_DP, 0.0)
        G.synchronize()
        rc, info = G.pres_solve(rel_tol=rel_tol, prec=prec, max_iter=5000)
        assert rc == 0 and info.converged == 1, (rc, info.as_dict())
        return info

    rows = {k: [] for k in ("stencil_constant_us", "stencil_variable_us", "residual_constant_us", "residual_variable_us", "direct_fused_isotropic_us", "direct_layered_us",
                            "fdm_apply_fused_isotropic_us", "fdm_apply_layered_5_launch_us", "line_solve_us")}
    iters = {}
    for key in ("general", "caprock"):
        for prec in ("fdm", "jacobi"):
            rows[f"{key}_{prec}_solve_us"] = []
    for run in range(a.runs + 1):                       # (run 0 warms up: tables, pivots, code objects)
        out = {}
        for name in ("constant", "layered"):            # alternating: constant, layered, constant, ...
            G = ctx[name]
            info = solve(G, pk.PREC_FDM, 1e-12)         # wall time without events ...
            assert info.iterations == 0
            G.timers_reset()                            # ... kernel times from a second solve with them
            solve(G, pk.PREC_FDM, 1e-12)
            for _ in range(3):
                G.pres_assemble_residual(1.0)
            G.synchronize()
            var = name == "layered"
            out["stencil_variable_us" if var else "stencil_constant_us"] = per_launch(G, "apply_p_stencil")
            out["residual_variable_us" if var else "residual_constant_us"] = per_launch(G, "pressure_residual")
            out["direct_layered_us" if var else "direct_fused_isotropic_us"] = 1e6 * info.seconds
            out["fdm_apply_layered_5_launch_us" if var else "fdm_apply_fused_isotropic_us"] = per_launch(G, "precondition_p_fdm_layered" if var else "precondition_p_fdm")
            if var:
                out["line_solve_us"] = per_launch(G, "q1_line_solve")
            G.timers_enable(0)
        for key in ("general", "caprock"):
            for prec, pid in (("fdm", pk.PREC_FDM), ("jacobi", pk.PREC_JACOBI)):
                info = solve(ctx[key], pid, 1e-8)
                iters[f"{key}_{prec}_iterations"] = int(info.iterations)
                out[f"{key}_{prec}_solve_us"] = 1e6 * info.seconds
        if run:
            for k, v in out.items():
                rows[k].append(v)
    kinds = {name: G.get_cell_permeability()[1] for name, G in ctx.items()}
    res = {"what": "per-cell permeability: variable-coefficient stencils and the line-solve form of PREC_FDM against their constant-coefficient counterparts",
           "box_cells": [n] * 3, "pressure_nodes": int(b.size), "runs": a.runs, "protocol": "median of the runs, variants alternating inside each run; max - min beside it; microseconds",
           "field_kinds": kinds, "iterations": iters, "times_us": {k: stats(v) for k, v in rows.items()}}
    for G in ctx.values():
        G.close()
    P.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"iterations": iters, "medians_us": {k: (v["median"] if v else None) for k, v in res["times_us"].items()}}))


if __name__ == "__main__":
    main()
