"""Per-cell permeability tensor on the MI355X: what the tensor instances of the per-cell stencils and of the line solve of PREC_FDM (k_p_stencil_cells<3, 3>,
k_p_residual_stencil_cells<3, 3>, k_q1_line_solve<3, 2>) cost next to the one-weight instances (<3, 1>), timed in the same session.  Writes profiles/permeability_tensor.json.

    python tools/permeability_tensor_bench.py [--cells 72] [--runs 5] [--out profiles/permeability_tensor.json]

Protocol (as tools/permeability_bench.py): every figure is the median of `runs` runs, scalar and tensor alternating inside each run, with max - min beside it.
Kernel times are HIP-event times per launch from the context's timers (poro_timers_get), solve times the wall time poro_pres_solve reports.
Material: biot_M = 1, k / mu = 1, dt = 1 on cells of edge 1.  The scalar field is the tensor's x component, so that both systems are of the same size."""
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


def layer_tables(n):
    k = np.arange(n)
    return np.stack([10.0 ** (-3 + 3 * ((7 * k) % 5) / 4), 10.0 ** (-3 + 3 * ((3 * k + 2) % 5) / 4), 10.0 ** (-3 + 3 * ((2 * k + 1) % 5) / 4)], axis=1)


def general_field(n):
    k, j, i = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    L = layer_tables(n)
    return np.stack([(L[k, d] * (1 + 0.5 * np.sin(1.7 * i + 2.3 * j + 0.9 * k + d))).ravel() for d in range(3)], axis=1)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "permeability_tensor.json"))
    a = ap.parse_args()
    n = a.cells
    P = pk.Problem.box(3, [n] * 3, [float(n)] * 3, 1, material(), [(0, 0, 0.0), (2, 1, 0.0), (4, 2, 0.0)])
    layered = np.repeat(layer_tables(n), n * n, axis=0)
    general = general_field(n)
    ctx = {}
    for name, f in (("scalar_layered", layered[:, 0]), ("tensor_layered", layered), ("scalar_general", general[:, 0]), ("tensor_general", general)):
        G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
        if f.ndim == 1:
            G.set_cell_permeability(f)
        else:
            G.set_cell_permeability_tensor(f)
        G.pres_assemble_jacobian(1.0)
        ctx[name] = G
    rng = np.random.default_rng(1)
    b = rng.standard_normal(ctx["scalar_layered"].n_p)
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

    names = ("operator_us", "residual_us", "line_solve_us", "fdm_apply_us", "direct_solve_us", "general_fdm_solve_us", "general_jacobi_solve_us")
    rows = {f"{kind}_{k}": [] for kind in ("scalar", "tensor") for k in names}
    iters = {}
    for run in range(a.runs + 1):                       # (run 0 warms up: tables, pivots, code objects)
        out = {}
        for kind in ("scalar", "tensor"):               # alternating: scalar, tensor, scalar, ...
            G = ctx[kind + "_layered"]
            info = solve(G, pk.PREC_FDM, 1e-12)         # wall time without events ...
            assert info.iterations == 0
            G.timers_reset()                            # ... kernel times from a second solve with them
            solve(G, pk.PREC_FDM, 1e-12)
            for _ in range(3):
                G.pres_assemble_residual(1.0)
            G.synchronize()
            out[f"{kind}_operator_us"] = per_launch(G, "apply_p_stencil")
            out[f"{kind}_residual_us"] = per_launch(G, "pressure_residual")
            out[f"{kind}_line_solve_us"] = per_launch(G, "q1_line_solve")
            out[f"{kind}_fdm_apply_us"] = per_launch(G, "precondition_p_fdm_layered")
            out[f"{kind}_direct_solve_us"] = 1e6 * info.seconds
            G.timers_enable(0)
            for prec, pid in (("fdm", pk.PREC_FDM), ("jacobi", pk.PREC_JACOBI)):
                info = solve(ctx[kind + "_general"], pid, 1e-8)
                iters[f"{kind}_general_{prec}_iterations"] = int(info.iterations)
                out[f"{kind}_general_{prec}_solve_us"] = 1e6 * info.seconds
        if run:
            for k, v in out.items():
                rows[k].append(v)
    kinds = {name: (G.get_cell_permeability_tensor() if name.startswith("tensor") else G.get_cell_permeability())[1] for name, G in ctx.items()}
    times = {k: stats(v) for k, v in rows.items()}
    ratio = {k: times["tensor_" + k]["median"] / times["scalar_" + k]["median"] for k in names if times["tensor_" + k] and times["scalar_" + k]}
    res = {"what": "per-cell permeability tensor: the tensor stencils and the tensor line solve of PREC_FDM against the scalar per-cell kernels, same session",
           "box_cells": [n] * 3, "pressure_nodes": int(b.size), "runs": a.runs, "protocol": "median of the runs, scalar and tensor alternating inside each run; max - min beside it; microseconds",
           "field_kinds": kinds, "iterations": iters, "times_us": times, "tensor_over_scalar": ratio}
    for G in ctx.values():
        G.close()
    P.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"iterations": iters, "medians_us": {k: (v["median"] if v else None) for k, v in times.items()}, "tensor_over_scalar": ratio}))


if __name__ == "__main__":
    main()
