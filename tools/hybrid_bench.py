"""The matrix-free displacement operator on a refined 3D box (cells [n/4, 3n/4)^3 split once by default: the mesh of tools/refined_step.py), in the general form
(the general cell kernels over every cell) or the hybrid form (poro_ctx_set_operator_form: the coarse box's structured kernel, minus the element products of the
refined box cells, plus the general kernels over the fine cells only) - the refined-box twin of tools/mfg_bench.py.  Prints seconds per application from
bench_operator, the cell-kernel launches per application and the cell counts from the getter.
Usage: python tools/hybrid_bench.py [coarse cells per direction = 32] [degree = 2] [--refined-fraction f] [--operator general|hybrid] [--scatter coloured|atomic]
--refined-fraction f: a centred block of about f of the coarse cells is refined instead (0 = the all-zero mask: the uniform box as a general mesh, 1 = every cell)"""
import argparse
import json, os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R]
import numpy as np
import poroelasticity_dealii_amd as pk
import bench

ap = argparse.ArgumentParser()
ap.add_argument("n", nargs="?", type=int, default=32); ap.add_argument("degree", nargs="?", type=int, default=2)
ap.add_argument("--refined-fraction", type=float, default=None); ap.add_argument("--operator", choices=["general", "hybrid"], default="general")
ap.add_argument("--scatter", choices=["coloured", "atomic"], default="coloured")
args = ap.parse_args()
n, deg = args.n, args.degree
mask = np.zeros((n, n, n), dtype=np.int32)
if args.refined_fraction is None:
    lo, hi = n // 4, 3 * n // 4
else:
    w = min(n, int(round(n * max(0.0, args.refined_fraction) ** (1.0 / 3.0)))); lo = (n - w) // 2; hi = lo + w
mask[lo:hi, lo:hi, lo:hi] = 1
P = pk.Problem.refined_box_mask(3, [n] * 3, [10.0] * 3, deg, bench.material(), bench.BC_3D, mask)
G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
G.fill(pk.VEC_P, 0.0); G.disp_assemble_system(True)
G.set_scatter_mode(pk.SCATTER_ATOMIC if args.scatter == "atomic" else pk.SCATTER_COLOURED)
G.set_operator_form(pk.OPFORM_HYBRID if args.operator == "hybrid" else pk.OPFORM_GENERAL)
t = G.bench_operator(pk.OP_MATRIX_FREE, int(os.environ.get("REPS", "20")))
G.timers_reset(); G.apply(pk.MAT_A_U, np.zeros(G.n_u)); launches = G.timer("mfg_cell_kernels")[1]; box_s = G.timer("apply_u_hybrid_box")[0]; G.timers_enable(0)
form, general_cells, removed = G.get_operator_form()
rec = {"mesh": f"box {n}^3 coarse cells Q{deg}, cells [{lo}, {hi})^3 refined once, no box tag", "N_u": int(G.n_u), "n_cells": int(P.desc.n_cells), "refined_coarse_cells": int(mask.sum()),
       "operator": args.operator, "scatter": args.scatter, "seconds_per_application": t, "DoF_updates_per_s": G.n_u / t, "cell_kernel_launches_per_application": int(launches),
       "general_cells_per_application": int(general_cells), "removed_box_cells": int(removed), "hybrid_box_part_seconds_one_application": box_s,
       "note": "time = HIP events over back-to-back applications incl. the memset of y; the box part (gather, structured kernel, removed cells + combine) from one event-timed application"}
print(json.dumps(rec))
G.close(); P.close()
