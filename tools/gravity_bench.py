"""Gravity on the MI355X: what the record needs besides the tests.  Writes profiles/gravity.json.

    python tools/gravity_bench.py [--parent DIR] [--n 72] [--q1 99] [--runs 5] [--steps 3] [--out profiles/gravity.json]

default_unchanged (only with --parent DIR, a built checkout of the parent commit): `python bench.py --gpus 1 --steps 4 --warmup 1` in DIR and in this tree, alternating,
    `runs` runs each, as fresh processes; the arrays of --dump-outputs of the first pair are compared bit for bit.  The rule (profiles/moduli_structured_default_unchanged.json):
    the difference of the medians of ms_per_step lies inside the parent's max - min.
zero_step_cost: the benchmark's time step at n^3 Q2, matrix-free, block FDM, on two runners of the same build - one without gravity, one with g = (0, 0, -9.81), a
    per-cell bulk density and a fluid density - alternating, `runs` runs of `steps` repeated steps each with events on every launch of the two timer families that read
    the folded vectors, assemble_u_rhs and pressure_residual (microseconds per launch).  The rule: the medians differ by no more than the without-gravity runs' max - min.
setup_kernels: microseconds of the four set-up kernels, HIP events around their launches (timer families gravity_body_u, gravity_flux_p): the two box kernels on the
    box-tagged context, the two cell-loop kernels (all colours of the coloured loop together, with the memset in front) on the same mesh without the box tag; per-cell
    density, and the flux with the scalar, the per-cell and the tensor permeability.  Medians of `runs` with max - min, recorded without a target."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

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


def zero_step_cost(n, runs, steps):
    families = ("assemble_u_rhs", "pressure_residual")
    runners = {}
    for name in ("without", "with"):
        P = pk.Problem.box(3, [n] * 3, [10.0] * 3, 2, material(), BC)
        kw = {}
        if name == "with":
            kw = dict(gravity=G, fluid_density=1000.0, density=2000.0 + 700.0 * ((7 * np.arange(P.desc.n_cells)) % 11) / 10.0)
        R = pk.Runner(P, 0, pk.OP_MATRIX_FREE, p_init=10e6, dt=60.0, abs_u=1e-12, rel_u=1e-8, max_it=50000, prec=pk.PREC_FDM, reduction=True, **kw)
        R.initialize(); R.save_state(); R.step(restore=True)
        runners[name] = (P, R)
        progress("zero_step_cost: runner", name, "ready")
    assert runners["with"][1].ctx.get_gravity()[3] and not runners["without"][1].ctx.get_gravity()[3]
    rows = {}
    for run in range(runs + 1):                               # (run 0 warms up)
        for name in ("without", "with"):                      # alternating
            R = runners[name][1]
            R.ctx.timers_reset(); R.ctx.timers_enable(1)
            for _ in range(steps):
                R.step(restore=True)
            R.ctx.timers_enable(0)
            for fam in families:
                sec, launches = R.ctx.timer(fam)
                if run:
                    rows.setdefault(f"{fam}_{name}_us", []).append(1e6 * sec / launches)
    t = {k: stats(v) for k, v in rows.items()}
    verdict = {fam: bool(abs(t[f"{fam}_with_us"]["median"] - t[f"{fam}_without_us"]["median"]) <= t[f"{fam}_without_us"]["max_minus_min"]) for fam in families}
    for P, R in runners.values():
        R.close(); P.close()
    return {"box_cells": [n] * 3, "degree": 2, "steps_per_run": steps, "microseconds_per_launch": t, "medians_differ_by_no_more_than_the_without_spread": verdict}


def setup_kernels(n, deg, runs):
    P = pk.Problem.box(3, [n] * 3, [10.0] * 3, deg, material(), BC)
    nc = P.desc.n_cells
    rho = 2000.0 + 700.0 * ((7 * np.arange(nc)) % 11) / 10.0
    k0 = P.desc.mat.k_over_mu
    kap = k0 * (1.0 + ((3 * np.arange(nc)) % 7) / 7.0)
    ten = np.stack([kap, 0.5 * kap, 2.0 * kap], axis=1)
    out = {"box_cells": [n] * 3, "degree": deg, "displacement_dofs": int(P.desc.n_dofs_u), "pressure_dofs": int(P.desc.n_dofs_p)}
    for label, problem in (("box", P), ("cell_loop", Untagged(P))):
        ctx = pk.Context(problem, 0, pk.OP_MATRIX_FREE)
        ctx.set_cell_density(rho)
        rows = {}
        for form, setter, value in (("scalar", ctx.set_cell_permeability, None), ("cell", ctx.set_cell_permeability, kap), ("tensor", ctx.set_cell_permeability_tensor, ten)):
            ctx.set_gravity(None, 0.0, 0.0)
            setter(value)
            for run in range(runs + 1):                       # (run 0 warms up)
                ctx.set_gravity(None, 0.0, 0.0)
                ctx.timers_reset(); ctx.timers_enable(1)
                ctx.set_gravity(G, 2700.0, 1000.0)            # one launch of either family (the cell loop: one per colour)
                ctx.timers_enable(0)
                if run:
                    rows.setdefault(f"flux_p_{form}_us", []).append(1e6 * ctx.timer("gravity_flux_p")[0])
                    if form == "scalar":
                        rows.setdefault("body_u_us", []).append(1e6 * ctx.timer("gravity_body_u")[0])
        out[label] = {k: stats(v) for k, v in rows.items()}
        progress("setup_kernels:", n, "cells, degree", deg, label, {k: v["median"] for k, v in out[label].items()})
        ctx.close()
    P.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (its own bench.py and package); without it the default_unchanged block is skipped")
    ap.add_argument("--n", type=int, default=72)
    ap.add_argument("--q1", type=int, default=99)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--skip", nargs="*", default=[], choices=["zero_step_cost", "setup_kernels"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gravity.json"))
    a = ap.parse_args()
    res = {}
    if os.path.exists(a.out):                                  # blocks measured by an earlier call stay
        with open(a.out) as f:
            res = json.load(f)
    res["what"] = ("gravity (body force and Darcy gravity flux, folded into constant vectors at set-up): the default against the parent commit, the cost on the time step, "
                   "and the set-up kernels; one MI355X")
    res["protocol"] = f"medians of {a.runs} runs, the variants alternating inside each run, max - min beside them"
    if a.parent:
        res["default_unchanged"] = default_unchanged(os.path.abspath(a.parent), a.runs)
    if "zero_step_cost" not in a.skip:
        res["zero_step_cost"] = zero_step_cost(a.n, a.runs, a.steps)
    if "setup_kernels" not in a.skip:
        res["setup_kernels"] = [setup_kernels(a.n, 2, a.runs), setup_kernels(a.q1, 1, a.runs)]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    brief = {k: v for k, v in res.items() if k in ("zero_step_cost", "setup_kernels")}
    if "default_unchanged" in res:
        brief["default_unchanged"] = {k: v for k, v in res["default_unchanged"].items() if k != "result_lines"}
    print(json.dumps(brief))


if __name__ == "__main__":
    main()
