"""Flow post-processing on the MI355X: what the record needs besides the tests.  Writes profiles/darcy_flux.json.

    python tools/darcy_flux_bench.py [--parent DIR] [--n 72] [--runs 5] [--out profiles/darcy_flux.json]

default_unchanged (only with --parent DIR, a built checkout of the parent commit): `python bench.py --gpus 1 --steps 4 --warmup 1` in DIR and in this tree, alternating,
    `runs` runs each, as fresh processes; the arrays of --dump-outputs of the first pair are compared bit for bit.  The rule: the difference of the medians of
    ms_per_step lies inside the parent's max - min.
kernels: at n^3 Q2, matrix-free, per-cell permeability, g = (0, 0, -9.81) with a fluid density and the top face drained: microseconds (HIP events, timer families
    of include/poroel_hip.h) of k_darcy_cells (family "darcy" of a velocity call), k_darcy_bfaces, k_darcy_label_sums (six labels), k_flow_balance with its
    finish ("flow_balance_sums"), of the whole enqueued sequence of one poro_pres_flow_balance call ("flow_balance"), of the wall time of that call with its copies
    and its synchronisation, and of the pressure_residual launch of the same context; on the box-tagged context and on the same mesh without the box tag.
    Medians of `runs` with max - min, recorded without a target."""
import argparse
import ctypes as C
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
G = [0.0, 0.0, -9.81]


def material():
    return pk.read_input(os.path.join(ROOT, "tests", "golden", "input.data")).material


def progress(*what):
    print(*what, file=sys.stderr, flush=True)


def stats(v):
    return {"median": float(np.median(v)), "max_minus_min": float(max(v) - min(v)), "runs": [float(x) for x in v]}


class Untagged:
    """the same mesh without the box and tensor tags: the general kernels run on it (a descriptor copy that shares every array with the source)"""

    def __init__(self, problem):
        self.source = problem
        self.desc = pk.Desc.from_buffer_copy(problem.desc)
        self.desc.box.enabled = 0
        self.desc.tensor.enabled = 0
        self.desc_ptr = C.pointer(self.desc)


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


def kernels(n, runs):
    P = pk.Problem.box(3, [n] * 3, [10.0] * 3, 2, material(), BC)
    P.set_pressure_bc([(5, 0.0)])
    nc, npd = P.desc.n_cells, P.desc.n_dofs_p
    kap = P.desc.mat.k_over_mu * (1.0 + ((3 * np.arange(nc)) % 7) / 7.0)
    rng = np.random.default_rng(1)
    out = {"box_cells": [n] * 3, "degree": 2, "cells": int(nc), "boundary_faces": int(P.desc.n_bfaces), "pressure_dofs": int(npd), "prescribed_dofs": int(P.desc.n_dirichlet_p)}
    for label, problem in (("box", P), ("cell_loop", Untagged(P))):
        ctx = pk.Context(problem, 0, pk.OP_MATRIX_FREE)
        ctx.set_cell_permeability(kap)
        ctx.set_gravity(G, 2700.0, 1000.0)
        for which in (pk.VEC_P, pk.VEC_P_OLD):
            ctx.set(which, 1e6 * rng.random(npd))
        for which in (pk.VEC_EPSV, pk.VEC_EPSV0):
            ctx.set(which, 1e-4 * rng.random(npd))
        rows = {}
        for run in range(runs + 1):                           # (run 0 warms up and builds the scratch)
            ctx.timers_reset(); ctx.timers_enable(1)
            ctx.darcy_velocity()
            ctx.timers_enable(0)
            cells_us = 1e6 * ctx.timer("darcy")[0]
            ctx.timers_reset(); ctx.timers_enable(1)
            ctx.boundary_discharge(list(range(6)))
            t0 = time.perf_counter(); ctx.flow_balance(60.0); wall = time.perf_counter() - t0
            ctx.pres_assemble_residual(60.0)
            ctx.timers_enable(0)
            if run:
                rows.setdefault("k_darcy_cells_us", []).append(cells_us)
                for fam, key in (("darcy_bfaces", "k_darcy_bfaces_us"), ("darcy_label_sums", "k_darcy_label_sums_us"), ("flow_balance_sums", "k_flow_balance_and_finish_us"),
                                 ("flow_balance", "flow_balance_enqueued_sequence_us"), ("pressure_residual", "pressure_residual_us")):
                    sec, launches = ctx.timer(fam)
                    rows.setdefault(key, []).append(1e6 * sec / max(1, launches))
                rows.setdefault("flow_balance_call_wall_us", []).append(1e6 * wall)
        out[label] = {k: stats(v) for k, v in rows.items()}
        progress("kernels:", n, "cells", label, {k: round(v["median"], 2) for k, v in out[label].items()})
        ctx.close()
    P.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (its own bench.py and package); without it the default_unchanged block is skipped")
    ap.add_argument("--n", type=int, default=72)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--skip", nargs="*", default=[], choices=["kernels"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "darcy_flux.json"))
    a = ap.parse_args()
    res = {}
    if os.path.exists(a.out):                                  # blocks measured by an earlier call stay
        with open(a.out) as f:
            res = json.load(f)
    res["what"] = "flow post-processing (Darcy velocity, boundary discharge, fluid mass balance): the default against the parent commit and the cost of the new kernels; one MI355X"
    res["protocol"] = f"medians of {a.runs} runs, max - min beside them; parent and head alternate inside each run"
    if a.parent:
        res["default_unchanged"] = default_unchanged(os.path.abspath(a.parent), a.runs)
    if "kernels" not in a.skip:
        res["kernels"] = kernels(a.n, a.runs)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    brief = {k: v for k, v in res.items() if k == "kernels"}
    if "default_unchanged" in res:
        brief["default_unchanged"] = {k: v for k, v in res["default_unchanged"].items() if k != "result_lines"}
    print(json.dumps(brief))


if __name__ == "__main__":
    main()
