"""Per-cell elastic moduli on the MI355X: what the per-cell pair costs the general cell kernel, what a box pays for leaving the structured kernel, what the line solve
of PREC_FDM costs next to the transform pair it stands in for, and a caprock case with the three displacement preconditioners.  Writes profiles/moduli_layered.json.

    python tools/moduli_bench.py [--cells 72 48] [--runs 5] [--out profiles/moduli_layered.json]

Protocol (as the project's other profiles): every figure is the median of `runs` runs, the variants alternating inside each run, with max - min beside it.
Operator times: poro_bench_operator (HIP events around `reps` applications).  Preconditioner times: poro_apply_preconditioner_u (HIP events around `reps` applications),
the line solve alone from the context's timer family fdm_u_line_solve.  Solve times: the wall time poro_disp_solve reports, tolerance 1e-8 ||rhs||."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import poroelasticity_dealii_amd as pk  # noqa: E402

BC = [(0, 0, 0.0), (1, 0, 0.0), (2, 1, 0.0), (3, 1, 0.0), (4, 2, 0.0), (5, 2, 0.0)]      # the faces of input.data: x faces fix u_x, y faces u_y, z faces u_z


def material():
    return pk.read_input(os.path.join(ROOT, "tests", "golden", "input.data")).material


def stats(v):
    v = [x for x in v if x is not None]
    return {"median": float(np.median(v)), "max_minus_min": float(max(v) - min(v)), "runs": [float(x) for x in v]} if v else None


def measure(n, runs, reps):
    m = material()
    box = pk.Problem.box(3, [n] * 3, [10.0] * 3, 2, m, BC)
    grid = pk.Problem.graded_box(3, [n] * 3, [10.0] * 3, 2, m, BC, [0.0] * 3)                # uniform tensor grid without the box tag: the general kernel without a field
    nc = box.desc.n_cells
    layer = np.arange(nc) // (n * n)
    const = (np.full(nc, m.lame_lambda), np.full(nc, m.shear_G))
    dec = 10.0 ** (-3 * ((7 * np.arange(n)) % 5) / 4)
    layered = (m.lame_lambda * dec[layer], m.shear_G * dec[layer])
    cap = np.where(layer >= n - n // 6, 100.0, 1.0)
    caprock = (m.lame_lambda * cap, m.shear_G * cap)
    ctx = {}

    def make(name, P, field, env=None):
        for k, v in (env or {}).items():
            os.environ[k] = v
        C = pk.Context(P, 0, pk.OP_MATRIX_FREE)
        if field is not None:
            C.set_cell_moduli(*field)
        C.set(pk.VEC_P, 1e7 * (1 + 0.2 * np.sin(0.37 * np.arange(C.n_p))))
        C.disp_assemble_system(True)
        if name.startswith("box"):
            C.apply_preconditioner_u(pk.PREC_FDM, np.ones(C.n_u))      # builds the tables in the form the environment selects
        for k in (env or {}):
            del os.environ[k]
        ctx[name] = C
    make("grid_scalar", grid, None)
    make("grid_field", grid, const)
    make("box_scalar", box, None)
    make("box_scalar_nodal", box, None, {"PORO_FDMU_NO_OCT": "1"})
    make("box_layered", box, layered)
    make("box_caprock", box, caprock)
    g = np.sin(0.37 * np.arange(ctx["box_scalar"].n_u) + 0.4)
    rows = {}

    def put(k, v):
        rows.setdefault(k, []).append(v)
    iters = {}
    for run in range(runs + 1):                             # (run 0 warms up)
        out = {}
        for name in ("grid_scalar", "grid_field", "box_scalar", "box_layered"):          # alternating
            out[f"operator_{name}_us"] = 1e6 * ctx[name].bench_operator(pk.OP_MATRIX_FREE, reps)
        for name in ("box_scalar", "box_scalar_nodal", "box_layered"):
            C = ctx[name]
            if name == "box_layered":
                C.timers_reset()
            out[f"fdm_apply_{name}_us"] = 1e6 * C.apply_preconditioner_u(pk.PREC_FDM, g, reps)[1]
            if name == "box_layered":
                C.synchronize()
                s, cnt = C.timer("fdm_u_line_solve")
                out["line_solve_us"] = 1e6 * s / cnt if cnt else None
                C.timers_enable(0)
        for prec, pid in (("fdm", pk.PREC_FDM), ("chebyshev", pk.PREC_CHEBYSHEV), ("jacobi", pk.PREC_JACOBI)):
            C = ctx["box_caprock"]
            C.fill(pk.VEC_U, 0.0); C.synchronize()
            rc, info = C.disp_solve(abs_tol=0.0, rel_tol=1e-8, max_iter=50000, prec=pid)
            assert rc == 0, (prec, info.as_dict())
            iters[f"caprock_{prec}_iterations"] = int(info.iterations)
            out[f"caprock_{prec}_solve_ms"] = 1e3 * info.seconds
        if run:
            for k, v in out.items():
                put(k, v)
    kinds = {name: C.get_cell_moduli()[2] for name, C in ctx.items()}
    res = {"box_cells": [n] * 3, "displacement_dofs": int(g.size), "field_kinds": kinds, "iterations": iters, "times": {k: stats(v) for k, v in rows.items()}}
    for C in ctx.values():
        C.close()
    box.close(); grid.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs="+", default=[72, 48])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moduli_layered.json"))
    a = ap.parse_args()
    res = {"what": "per-cell elastic moduli: the general cell kernel with and without the per-cell pair, a box on the general kernel against the structured one, the line-solve "
                   "form of PREC_FDM against the nodal and the octant isotropic forms, a caprock case (the top sixth of the layers 100 x stiffer) with three preconditioners",
           "runs": a.runs, "reps_per_timing": a.reps, "protocol": "median of the runs, variants alternating inside each run; max - min beside it; Q2 / Q1, one MI355X",
           "sizes": [measure(n, a.runs, a.reps) for n in a.cells]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for s in res["sizes"]:
        print(json.dumps({"cells": s["box_cells"][0], "iterations": s["iterations"], "medians": {k: (v["median"] if v else None) for k, v in s["times"].items()}}))


if __name__ == "__main__":
    main()
