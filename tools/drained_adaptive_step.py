"""Step time and pressure CG iterations per step of a drained adaptive column (Terzaghi's problem, corrected fixed-stress loop) at a size where the host driver picks the
two-level form for the pressure system (>= 4096 pressure dofs), against Jacobi on the pressure system (jacobi_p).  Every run: initialize, two steps, adapt, one warm step,
then `--steps` timed steps; `--runs` alternating runs of the two variants, medians reported.
Usage: python tools/drained_adaptive_step.py [nx ny nz] [--runs 5] [--steps 3] > out.json"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path[:0] = [ROOT]
import numpy as np
import poroelasticity_dealii_amd as pk
import bench

ap = argparse.ArgumentParser(); ap.add_argument("n", nargs="*", type=int); ap.add_argument("--runs", type=int, default=5); ap.add_argument("--steps", type=int, default=3)
args = ap.parse_args()
n = args.n or [16, 16, 64]
H, SIGMA0, DT = 10.0, 1.0e6, 60.0
m = bench.material(); m.flow_rate = 0.0
Kv = m.lame_lambda + 2 * m.shear_G
p0 = (m.biot_alpha * SIGMA0 / Kv) / (m.biot_alpha ** 2 / Kv + 1.0 / m.biot_M)                      # the undrained response
bc = [(0, 0, 0.0), (2, 1, 0.0), (1, 0, 0.0), (3, 1, 0.0), (4, 2, 0.0)]                           # rollers on the sides and the bottom
P = pk.Problem.refined_box_mask(3, n, [10.0, 10.0, H], 1, m, bc, np.zeros(int(np.prod(n)), dtype=np.int32), [(5, 2, -SIGMA0)])
P.set_pressure_bc([(5, 0.0)])                                                                     # drained top
names = {0: "none", 1: "Jacobi", 3: "FDM", 6: "two-level"}
runs = {"two_level_p": [], "jacobi_p": []}
for r in range(args.runs):
    for name, jp in (("two_level_p", False), ("jacobi_p", True)):
        R = pk.Runner(P, 0, pk.OP_MATRIX_FREE, p_init=p0, dt=DT, max_fss=200, max_it=50000, prec=-1, jacobi_p=jp, coupled_fss=True, incremental_strain=True)
        R.initialize(); R.step(); R.step()
        before, after = R.adapt()
        assert R.preconditioners()[1] == (pk.PREC_JACOBI if jp else pk.PREC_TWO_LEVEL), R.preconditioners()      # what the driver picked on the adapted mesh
        R.step(); R.ctx.synchronize()
        w0 = R.work(); t0 = time.perf_counter(); rows = 0
        for _ in range(args.steps):
            tr, _w = R.step(); rows += len(tr)
        R.ctx.synchronize(); sec = (time.perf_counter() - t0) / args.steps; w1 = R.work()
        runs[name].append({"ms_per_step": 1e3 * sec, "cg_p_per_step": (w1["cg_p"] - w0["cg_p"]) / args.steps, "cg_u_per_step": (w1["cg_u"] - w0["cg_u"]) / args.steps,
                           "fss_iterations_per_step": rows / args.steps, "cells": [int(before), int(after)], "n_dofs_p": int(R.problem.desc.n_dofs_p), "hanging_p": int(R.problem.desc.cons_p.n), "preconditioner_p": names[R.preconditioners()[1]]})
        R.close()
out = {"mesh": f"drained column, {n} coarse cells, 3D Q1/Q1, all-zero mask, one adapt before step 3 (fractions 0.6 / 0.4), dt = {DT} s", "timed_steps_per_run": args.steps, "runs": args.runs,
       "median": {k: {f: statistics.median(x[f] for x in v) for f in ("ms_per_step", "cg_p_per_step", "cg_u_per_step", "fss_iterations_per_step")} for k, v in runs.items()},
       "all": runs}
P.close()
print(json.dumps(out, indent=1))
