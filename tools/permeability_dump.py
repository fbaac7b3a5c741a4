"""Per-cell permeability, scalar and diagonal tensor: everything the pressure system computes from a field on small boxes, written into one .npz so that two builds of the
library can be compared bit for bit.  Public Python API only.

    python tools/permeability_dump.py --out A.npz
    python tools/permeability_dump.py --compare A.npz B.npz [--report report.json]

Boxes (1,1), (7,5), (1,1,1), (2,1,3), (5,4,6), (9,8,7); {scalar, tensor} x {layered, general} fields; operator forms CSR and matrix-free; the layered fields also with the
low face of the slowest direction prescribed, and with both of its faces.  Per case: the exported Jacobian values, pres_apply_jacobian(x), the pressure residual, and dp,
iteration count and return code of pres_solve(prec=PREC_FDM) - then the same once more after set_cell_permeability*(None).
Material, fields, x and states as in tests/test_permeability_tensor_gpu.py: biot_M = 1, k / mu = 1, dt = 1 on cells of edge 1, kappa_d(c) = L_d[k] (1 + 0.5 sin(1.7 i +
2.3 j + 0.9 k + d)); the scalar field is the tensor's x component.  --compare reports np.array_equal per entry and leaves with status 1 if any entry differs."""
import argparse
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DT = 1.0
BOXES = [(1, 1), (7, 5), (1, 1, 1), (2, 1, 3), (5, 4, 6), (9, 8, 7)]


def L_H0(k): return 10.0 ** (-3 + 3 * ((7 * int(k)) % 5) / 4)
def L_H1(k): return 10.0 ** (-3 + 3 * ((3 * int(k) + 2) % 5) / 4)
def L_V(k): return 10.0 ** (-3 + 3 * ((2 * int(k) + 1) % 5) / 4)


def box_field(n, layered_only):
    """(n_cells, dim) in lattice cell order (x fastest); k = the index along the slowest direction"""
    dim = len(n)
    tables = [L_H0, L_V] if dim == 2 else [L_H0, L_H1, L_V]
    out = np.empty((int(np.prod(n)), dim))
    for c, idx in enumerate(itertools.product(*[range(m) for m in n[::-1]])):
        ijk = list(idx[::-1]) + [0] * (3 - dim)
        for d, L in enumerate(tables):
            out[c, d] = L(ijk[dim - 1]) * (1.0 if layered_only else 1 + 0.5 * np.sin(1.7 * ijk[0] + 2.3 * ijk[1] + 0.9 * ijk[2] + d))
    return out


def observe(pk, G, x, b, rel_tol, out, key):
    """the Jacobian's values, J x, the residual and the FDM solve of the context's present field"""
    G.pres_assemble_jacobian(DT)
    out[key + "/jacobian"] = G.export_csr(pk.MAT_JACOBIAN_P)[2]
    out[key + "/apply"] = G.pres_apply_jacobian(x)
    G.pres_assemble_residual(DT)
    out[key + "/residual"] = G.get(pk.VEC_RESIDUAL_P)
    if not G.supports_preconditioner(1, pk.PREC_FDM):
        out[key + "/solve"] = np.array([-1.0, -1.0])
        return
    G.set(pk.VEC_RESIDUAL_P, b); G.fill(pk.VEC_DP, 0.0)
    rc, info = G.pres_solve(rel_tol=rel_tol, prec=pk.PREC_FDM, max_iter=2000)
    out[key + "/dp"] = G.get(pk.VEC_DP)
    out[key + "/solve"] = np.array([float(rc), float(info.iterations)])


def dump(path):
    import poroelasticity_dealii_amd as pk
    m = pk.read_input(os.path.join(ROOT, "tests", "golden", "input.data")).material
    m.biot_M, m.k_over_mu, m.flow_rate = 1.0, 1.0, 0.0
    out = {}
    for n in BOXES:
        dim = len(n)
        for faces in ("free", "lo", "lohi"):
            P = pk.Problem.box(dim, list(n), [float(v) for v in n], 1, m, [(2 * d, d, 0.0) for d in range(dim)])
            if faces != "free":
                P.set_pressure_bc([(2 * dim - 2, 0.0)] + ([(2 * dim - 1, 0.0)] if faces == "lohi" else []))
            for mode, mname in ((pk.OP_CSR, "csr"), (pk.OP_MATRIX_FREE, "mf")):
                for layered in (True, False) if faces == "free" else (True,):
                    field = box_field(n, layered)
                    for kind in ("scalar", "tensor"):
                        key = f"{'x'.join(map(str, n))}/{faces}/{mname}/{kind}/{'layered' if layered else 'general'}"
                        G = pk.Context(P, 0, mode)
                        try:
                            st = np.random.default_rng(99)
                            for v in (pk.VEC_P, pk.VEC_P_OLD, pk.VEC_EPSV, pk.VEC_EPSV0):
                                G.set(v, st.standard_normal(G.n_p))
                            rng = np.random.default_rng(7 + dim + n[0])
                            x = rng.standard_normal(G.n_p); b = rng.standard_normal(G.n_p)
                            if kind == "scalar":
                                G.set_cell_permeability(field[:, 0].copy())
                            else:
                                G.set_cell_permeability_tensor(field)
                            observe(pk, G, x, b, 1e-12 if layered else 1e-8, out, key)
                            if kind == "scalar":
                                G.set_cell_permeability(None)
                            else:
                                G.set_cell_permeability_tensor(None)
                            observe(pk, G, x, b, 1e-12, out, key + "/constant_again")
                        finally:
                            G.close()
            P.close()
    np.savez(path, **out)
    print(f"{len(out)} entries -> {path}")


def compare(a, b, report):
    A, B = np.load(a), np.load(b)
    keys = sorted(set(A.files) | set(B.files))
    equal = {k: bool(k in A.files and k in B.files and np.array_equal(A[k], B[k])) for k in keys}
    differ = [k for k in keys if not equal[k]]
    res = {"what": "tools/permeability_dump.py --compare: np.array_equal per entry of two dumps", "entries": len(keys), "equal": len(keys) - len(differ), "differ": differ,
           "values": int(sum(A[k].size for k in A.files)), "per_entry": equal}
    if report:
        with open(report, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps({k: res[k] for k in ("entries", "equal", "differ", "values")}))
    return 1 if differ else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("A.npz", "B.npz"))
    ap.add_argument("--report")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(a.compare[0], a.compare[1], a.report))
    if not a.out:
        ap.error("--out or --compare")
    dump(a.out)
