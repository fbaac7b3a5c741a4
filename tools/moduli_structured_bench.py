"""Structured box operator for layered per-cell moduli on the MI355X (Context.set_moduli_operator): per application the cell loop with the layered field (same binary,
request off), the layered structured kernel, and the constant structured kernel without a field; a caprock solve (PREC_FDM, to 1e-8 ||rhs||) in both forms.
Writes profiles/moduli_structured.json.

    python tools/moduli_structured_bench.py [--q2 72 48] [--q1 99] [--runs 5] [--reps 20] [--out profiles/moduli_structured.json]

Protocol (as profiles/moduli_layered.json): every figure is the median of `runs` runs, the variants alternating inside each run, with max - min beside it.
Operator times: poro_bench_operator (HIP events around `reps` applications).  Solve times: the wall time poro_disp_solve reports.
The rule the result is judged by: a variant is faster when the drop of the median exceeds three times the slower variant's max - min."""
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
    return {"median": float(np.median(v)), "max_minus_min": float(max(v) - min(v)), "runs": [float(x) for x in v]}


def measure(n, deg, runs, reps, solves):
    m = material()
    box = pk.Problem.box(3, [n] * 3, [10.0] * 3, deg, m, BC)
    nc = box.desc.n_cells
    layer = np.arange(nc) // (n * n)
    dec = 10.0 ** (-3 * ((7 * np.arange(n)) % 5) / 4)
    layered = (m.lame_lambda * dec[layer], m.shear_G * dec[layer])
    cap = np.where(layer >= n - n // 6, 100.0, 1.0)
    caprock = (m.lame_lambda * cap, m.shear_G * cap)
    ctx = {}

    def make(name, field, form):
        C = pk.Context(box, 0, pk.OP_MATRIX_FREE)
        C.set_moduli_operator(form)
        if field is not None:
            C.set_cell_moduli(*field)
        C.set(pk.VEC_P, 1e7 * (1 + 0.2 * np.sin(0.37 * np.arange(C.n_p))))
        C.disp_assemble_system(True)
        want = form if field is not None else pk.MODULI_OP_CELLS
        assert C.get_moduli_operator() == (form, want), (name, C.get_moduli_operator())
        ctx[name] = C
    make("cell_loop", layered, pk.MODULI_OP_CELLS)
    make("structured", layered, pk.MODULI_OP_STRUCTURED)
    make("constant", None, pk.MODULI_OP_CELLS)
    if solves:
        make("caprock_cell_loop", caprock, pk.MODULI_OP_CELLS)
        make("caprock_structured", caprock, pk.MODULI_OP_STRUCTURED)
    rows, iters = {}, {}
    for run in range(runs + 1):                             # (run 0 warms up)
        out = {}
        for name in ("cell_loop", "structured", "constant"):                              # alternating
            out[f"operator_{name}_us"] = 1e6 * ctx[name].bench_operator(pk.OP_MATRIX_FREE, reps)
        for name in ("caprock_cell_loop", "caprock_structured") if solves else ():
            C = ctx[name]
            C.fill(pk.VEC_U, 0.0); C.synchronize()
            rc, info = C.disp_solve(abs_tol=0.0, rel_tol=1e-8, max_iter=50000, prec=pk.PREC_FDM)
            assert rc == 0, (name, info.as_dict())
            iters[f"{name}_iterations"] = int(info.iterations)
            out[f"{name}_solve_ms"] = 1e3 * info.seconds
        if run:
            for k, v in out.items():
                rows.setdefault(k, []).append(v)
    t = {k: stats(v) for k, v in rows.items()}
    cl, st, co = t["operator_cell_loop_us"], t["operator_structured_us"], t["operator_constant_us"]
    res = {"box_cells": [n] * 3, "degree": deg, "displacement_dofs": int(ctx["constant"].n_u), "iterations": iters, "times": t,
           "cell_loop_over_structured": cl["median"] / st["median"], "structured_over_constant": st["median"] / co["median"],
           "structured_beats_cell_loop_by_the_rule": bool(cl["median"] - st["median"] > 3 * cl["max_minus_min"])}
    for C in ctx.values():
        C.close()
    box.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--q2", type=int, nargs="*", default=[72, 48])
    ap.add_argument("--q1", type=int, nargs="*", default=[99])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moduli_structured.json"))
    a = ap.parse_args()
    res = {"what": "structured box operator for moduli layered along z (kernels_kron_lm.hip) against the general cell loop with the same field and against the constant "
                   "structured kernel without a field; a caprock case (the top sixth of the layers 100 x stiffer), PREC_FDM to 1e-8 ||rhs||, in both forms",
           "runs": a.runs, "reps_per_timing": a.reps, "protocol": "median of the runs, variants alternating inside each run; max - min beside it; one MI355X",
           "sizes": [measure(n, 2, a.runs, a.reps, True) for n in a.q2] + [measure(n, 1, a.runs, a.reps, False) for n in a.q1]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for s in res["sizes"]:
        print(json.dumps({"cells": s["box_cells"][0], "degree": s["degree"], "iterations": s["iterations"], "medians": {k: v["median"] for k, v in s["times"].items()},
                          "cell_loop_over_structured": s["cell_loop_over_structured"], "structured_over_constant": s["structured_over_constant"],
                          "beats_by_rule": s["structured_beats_cell_loop_by_the_rule"]}))


if __name__ == "__main__":
    main()
