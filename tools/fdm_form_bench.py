"""Block FDM of the displacement system on single-rank 3D boxes whose directions are not all mirror-symmetric: the nodal kernels (the default there) against the
per-direction form (poro_ctx_set_fdm_form, PORO_FDM_FORM_PER_DIRECTION).  Per shape and form: seconds per preconditioner application (apply_preconditioner_u(reps=...):
the transform sweeps alone, as inside PCG - the nodal kernels' five, the form's three; the form's butterflies ride in the CG vector kernels and show in the step time),
and the first time step through the host runner: wall seconds, the seconds of its displacement solves and their CG iterations.  Medians of --runs alternating runs
(nodal, form, nodal, form, ...) with the spread (min, max) next to every median; one JSON document on stdout, or in --out.
On a commit without the form (no pk.FDM_FORM_PER_DIRECTION) the nodal kernels alone are measured: the parent's side of the comparison.
Usage: python tools/fdm_form_bench.py [--runs 5] [--reps 20] [--shapes name,name,...] [--out FILE]"""
import argparse, json, os, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R]
import numpy as np
import poroelasticity_dealii_amd as pk
import bench

COLUMN = [(0, 0, 0.0), (1, 0, 0.0), (2, 1, 0.0), (3, 1, 0.0), (4, 2, 0.0)]          # consolidation column: rollers on the sides, held at the bottom
LOW_FACES = [(0, 0, 0.0), (2, 1, 0.0), (4, 2, 0.0)]
# name: (cells, degree, Dirichlet list, grading or None, what the form does there)
SHAPES = {
    "column_48_q2": ((48, 48, 48), 2, COLUMN, None, "z whole: 97, x and y half: 49"),
    "column_32x32x63_q2": ((32, 32, 63), 2, COLUMN, None, "z whole: 127, x and y half: 33"),
    "column_99_q1": ((99, 99, 99), 1, COLUMN, None, "z whole: 100, x and y half: 50"),
    "graded_z_48_q2": ((48, 48, 48), 2, bench.BC_3D, (0.0, 0.0, -0.7), "tensor-product grid graded in z: z whole 97, x and y half 49"),
    "low_faces_48_q2": ((48, 48, 48), 2, LOW_FACES, None, "mask (0, 0, 0): every direction whole, 97"),
}
HAVE_FORM = hasattr(pk, "FDM_FORM_PER_DIRECTION")


def stat(v):
    v = sorted(float(x) for x in v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "n": len(v)}


def measure(name, runs, reps):
    cells, deg, bc, grading, what = SHAPES[name]
    mat = bench.material()
    P = pk.Problem.box(3, list(cells), [10.0] * 3, deg, mat, bc) if grading is None else pk.Problem.graded_box(3, list(cells), [10.0] * 3, deg, mat, bc, list(grading))
    forms = ["nodal", "per_direction"] if HAVE_FORM else ["nodal"]
    rec = {"shape": name, "cells": list(cells), "degree": deg, "note": what, "forms": {}}
    # per application: one context per form, alternating
    ctx = {}
    for f in forms:
        G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
        if f == "per_direction":
            G.set_fdm_form(pk.FDM_FORM_PER_DIRECTION)
        G.fill(pk.VEC_P, 0.0); G.disp_assemble_system(True)
        ctx[f] = G
        rec["forms"][f] = {"apply_seconds": [], "step_seconds": [], "solve_u_seconds": [], "cg_iterations": []}
        if HAVE_FORM:
            req, eff, split = G.get_fdm_form()
            rec["forms"][f]["effective"] = {0: "nodal", 1: "octant", 2: "per_direction", 3: "slab", 4: "planar"}[eff]; rec["forms"][f]["split"] = list(split)
    rec["N_u"] = int(ctx["nodal"].n_u)
    g = np.random.default_rng(7).standard_normal(rec["N_u"])
    nd = P.desc.n_dirichlet
    g[np.ctypeslib.as_array(P.desc.dirichlet_dof, shape=(nd,))] = 0.0
    for f in forms:
        ctx[f].apply_preconditioner_u(pk.PREC_FDM, g, reps=3)       # warm-up
    for _ in range(runs):
        for f in forms:
            rec["forms"][f]["apply_seconds"].append(ctx[f].apply_preconditioner_u(pk.PREC_FDM, g, reps=reps)[1])
    for f in forms:
        ctx[f].close()
    # first time step through the host runner: restore-and-step repeats it from the same state
    run, last = {}, {}
    for f in forms:
        kw = {"fdm_per_direction": True} if f == "per_direction" else {}
        Rn = pk.Runner(P, prec=pk.PREC_FDM, max_it=2000, **kw)
        Rn.initialize(); Rn.save_state()
        _, last[f] = Rn.step()                                          # warm-up (builds the block FDM, fills the iteration hints); the work counters accumulate over the steps
        run[f] = Rn
    for _ in range(runs):
        for f in forms:
            Rn = run[f]
            Rn.ctx.synchronize(); t0 = time.perf_counter()
            trace, work = Rn.step(restore=True)
            Rn.ctx.synchronize(); dt = time.perf_counter() - t0
            F = rec["forms"][f]
            F["step_seconds"].append(dt); F["solve_u_seconds"].append((work["usec_solve_u"] - last[f]["usec_solve_u"]) * 1e-6); F["cg_iterations"].append(int(work["cg_u"] - last[f]["cg_u"]))
            last[f] = work
            F["fss_iterations"] = int(trace.shape[0])
    for f in forms:
        if f == "per_direction":
            rec["forms"][f]["solves_in_the_form"] = int(run[f].ctx.timer("fdm_u_per_direction_form")[1])
        run[f].close()
    for f in forms:
        F = rec["forms"][f]
        for k in ("apply_seconds", "step_seconds", "solve_u_seconds"):
            F[k] = stat(F[k])
        F["cg_iterations"] = sorted(set(F["cg_iterations"]))
    if HAVE_FORM:
        a, b = rec["forms"]["nodal"], rec["forms"]["per_direction"]
        rec["nodal_over_per_direction"] = {k: a[k]["median"] / b[k]["median"] for k in ("apply_seconds", "step_seconds", "solve_u_seconds")}
    P.close()
    return rec


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5); ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default=",".join(SHAPES)); ap.add_argument("--out", default=None)
    args = ap.parse_args()
    doc = {"tool": "tools/fdm_form_bench.py", "per_direction_form_available": HAVE_FORM, "runs": args.runs, "reps_per_application_timing": args.reps,
           "protocol": "medians of alternating runs (nodal, per-direction, nodal, ...), spread = (min, max); apply: HIP events over back-to-back applications; step: wall clock of the first "
                       "time step repeated from its restored state, solve_u: the displacement solves inside it",
           "shapes": []}
    for name in args.shapes.split(","):
        doc["shapes"].append(measure(name, args.runs, args.reps))
        print(json.dumps(doc["shapes"][-1]), file=sys.stderr, flush=True)
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)
