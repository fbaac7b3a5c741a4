"""Mechanical post-processing on the MI355X: what the record needs besides the tests.  Writes profiles/stress_postprocess.json.

    python tools/stress_bench.py [--parent DIR] [--runs 5] [--out profiles/stress_postprocess.json]

default_unchanged (only with --parent DIR, a built checkout of the parent commit): `python bench.py --gpus 1 --steps 4 --warmup 1` in DIR and in this tree, alternating,
    `runs` runs each, as fresh processes; the arrays of --dump-outputs of the first pair are compared bit for bit.  The rule: the medians agree within the parent's own
    max - min.
calls: at 72^3 Q2 with the material's scalars, at 72^3 Q2 with a 3-layer moduli field and at 99^3 Q1, matrix-free, block-FDM run, the state after one time step:
    microseconds of poro_disp_cell_stress, poro_disp_cell_measures (with a criterion) and poro_disp_force_balance (with the per-dof reactions), each split into the
    kernel time (HIP events, the timer families "cell_stress", "cell_measures", "force_balance") and the rest of the call's wall time - the device-to-host copies and the
    synchronisation; beside them, from the same process, the wall time of that time step and of one poro_get_effective_stresses with its projections
    (Runner.postprocess() without a directory).  Medians of `runs` with max - min, recorded without a target."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import poroelasticity_dealii_amd as pk  # noqa: E402

BC = [(0, 0, 0.0), (1, 0, -1e-5), (2, 1, 0.0), (3, 1, -1e-5), (4, 2, 0.0), (5, 2, -1e-5)]      # the benchmark's: input.data + the z faces


def inputs():
    return pk.read_input(os.path.join(ROOT, "tests", "golden", "input.data"))


def progress(*what):
    print(*what, file=sys.stderr, flush=True)


def stats(v):
    return {"median": float(np.median(v)), "max_minus_min": float(max(v) - min(v)), "runs": [float(x) for x in v]}


def default_unchanged(parent, runs):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "4", "--warmup", "1"]
    lines = {"parent": [], "head": []}
    equal = None
    with tempfile.TemporaryDirectory() as tmp:
        for run in range(runs):
            for who, cwd in (("parent", parent), ("head", ROOT)):
                extra = ["--dump-outputs", os.path.join(tmp, who)] if run == 0 else []
                out = subprocess.run(cmd + extra, cwd=cwd, check=True, capture_output=True, text=True, timeout=900).stdout
                lines[who].append(json.loads([l for l in out.splitlines() if l.startswith("{")][-1]))
                progress("default_unchanged: run", run, who, lines[who][-1]["ms_per_step"], "ms per step")
            if run == 0:
                names = sorted(os.listdir(os.path.join(tmp, "parent")))
                assert names == sorted(os.listdir(os.path.join(tmp, "head"))), names
                equal = {n: bool(open(os.path.join(tmp, "parent", n), "rb").read() == open(os.path.join(tmp, "head", n), "rb").read()) for n in names}
    ms = {who: stats([l["ms_per_step"] for l in lines[who]]) for who in lines}
    diff = ms["head"]["median"] - ms["parent"]["median"]
    return {"command": " ".join(cmd[1:]), "ms_per_step": ms, "difference_head_minus_parent": diff, "difference_inside_parent_spread": bool(abs(diff) <= ms["parent"]["max_minus_min"]),
            "dumped_outputs_bitwise_equal": equal, "result_lines": lines}


def layered(P):
    """three layers of z by cell centres: the material's moduli, a fifth and 3.5 times of them"""
    d = P.desc
    X = np.ctypeslib.as_array(d.vertex_coords, shape=(d.n_vertices, 3)); cv = np.ctypeslib.as_array(d.cell_vertices, shape=(d.n_cells, 8))
    z = X[cv][:, :, 2].mean(axis=1)
    layer = np.minimum(2, (3 * (z - X[:, 2].min()) / np.ptp(X[:, 2])).astype(int))
    return d.mat.lame_lambda * np.array([1.0, 0.2, 3.5])[layer], d.mat.shear_G * np.array([1.0, 0.3, 4.0])[layer]


def calls(n, degree, field, runs):
    I = inputs()
    P = pk.Problem.box(3, [n] * 3, [10.0] * 3, degree, I.material, BC)
    R = pk.Runner(P, 0, pk.OP_MATRIX_FREE, p_init=I.p_init, dt=I.time_step, abs_u=1e-12, rel_u=1e-8, max_it=50000, prec=pk.PREC_FDM, reduction=True)
    out = {"box_cells": [n] * 3, "degree": degree, "moduli": field, "cells": int(P.desc.n_cells), "displacement_dofs": int(P.desc.n_dofs_u), "dirichlet_dofs": int(P.desc.n_dirichlet)}
    try:
        R.initialize()
        R.step()                                                # (warm-up: tables, first launches)
        C = R.ctx
        rows = {}
        for run in range(runs):
            t0 = time.perf_counter(); R.step(); rows.setdefault("time_step_wall_us", []).append(1e6 * (time.perf_counter() - t0))
            t0 = time.perf_counter(); R.postprocess(); rows.setdefault("effective_stresses_with_projections_wall_us", []).append(1e6 * (time.perf_counter() - t0))
        if field == "layered":
            C.set_cell_moduli(*layered(P))
            C.disp_assemble_system(True)
        phi = np.deg2rad(30.0)
        for run in range(runs + 1):                             # (run 0 builds the scratch)
            for fam, call in (("cell_stress", C.cell_stress), ("cell_measures", lambda: C.cell_measures(cohesion=2.0e5, friction_angle=phi)), ("force_balance", C.force_balance)):
                C.timers_reset(); C.timers_enable(1)
                t0 = time.perf_counter(); call(); wall = 1e6 * (time.perf_counter() - t0)
                C.timers_enable(0)
                kern = 1e6 * C.timer(fam)[0]
                if run:
                    rows.setdefault(fam + "_kernels_us", []).append(kern)
                    rows.setdefault(fam + "_copies_and_sync_us", []).append(wall - kern)
                    rows.setdefault(fam + "_call_wall_us", []).append(wall)
        out.update({k: stats(v) for k, v in rows.items()})
        progress("calls:", n, "cells, degree", degree, field, {k: round(v["median"], 1) for k, v in out.items() if isinstance(v, dict)})
    finally:
        R.close(); P.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (its own bench.py and package); without it the default_unchanged block is skipped")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--skip", nargs="*", default=[], choices=["calls"])
    ap.add_argument("--q2", type=int, default=72)
    ap.add_argument("--q1", type=int, default=99)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stress_postprocess.json"))
    a = ap.parse_args()
    res = {}
    if os.path.exists(a.out):                                  # blocks measured by an earlier call stay
        with open(a.out) as f:
            res = json.load(f)
    res["what"] = "mechanical post-processing (cell stresses, failure measures, force balance): the default against the parent commit and the cost of the three calls; one MI355X"
    res["protocol"] = f"medians of {a.runs} runs, max - min beside them; parent and head alternate inside each run"
    if a.parent:
        res["default_unchanged"] = default_unchanged(os.path.abspath(a.parent), a.runs)
    if "calls" not in a.skip:
        res["calls"] = [calls(a.q2, 2, "scalar", a.runs), calls(a.q2, 2, "layered", a.runs), calls(a.q1, 1, "scalar", a.runs)]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    brief = {k: v for k, v in res.items() if k == "calls"}
    if "default_unchanged" in res:
        brief["default_unchanged"] = {k: v for k, v in res["default_unchanged"].items() if k != "result_lines"}
    print(json.dumps(brief))


if __name__ == "__main__":
    main()
