"""Shared problem definitions of the test-suite: the bundled input.data values (reference input.data:1-41),
committed here as numbers because /root/reference does not exist on the GPU box."""
import os
import subprocess

import numpy as np

import poroelasticity_dealii_amd as pk

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INPUT_DATA = os.path.join(GOLDEN, "input.data")       # byte copy of the reference's example parameter file (a data fixture)
DOMAIN_MSH = os.path.join(GOLDEN, "domain.msh")       # byte copy of the reference's example Gmsh mesh (a data fixture)

# derived constants of input.data
REF = dict(E=1.4e10, nu=0.3, alpha=0.9, poro=0.3, f_comp=5.8e-10, perm_mD=10.0, visc=1e-3, r_well=1.0, flow_rate=1e-5, p_init=10e6, dt=60.0)


def material(**over):
    import oracle_py
    d = dict(REF); d.update(over)
    g = oracle_py.derived_parameters(d["E"], d["nu"], d["alpha"], d["poro"], d["f_comp"], d["perm_mD"], d["visc"])
    return pk.Material(g["lambda"], g["G"], d["alpha"], g["K"], g["M"], g["k_over_mu"], d["r_well"], d["flow_rate"])


def host_material(path=None):
    """material through the product's own parameter front end"""
    return pk.read_input(path or INPUT_DATA).material


# input.data:14-16 (x faces fix u_x, y faces fix u_y); z faces per SURVEY Q9
BC_2D = [(0, 0, 0.0), (1, 0, -1e-5), (2, 1, 0.0), (3, 1, -1e-5)]
BC_3D = BC_2D + [(4, 2, 0.0), (5, 2, -1e-5)]


def box_problem(dim, n, degree, rank=0, n_ranks=1, mat=None, bc=None, neumann=()):
    n = [n] * dim if np.isscalar(n) else list(n)
    return pk.Problem.box(dim, n, [10.0] * dim, degree, mat or material(), bc if bc is not None else (BC_2D if dim == 2 else BC_3D), neumann, rank, n_ranks)


def node_coords_box(dim, n, degree, size=10.0):
    """coordinates of the lexicographic u nodes of the box"""
    n = [n] * dim if np.isscalar(n) else list(n)
    ax = [np.linspace(-size / 2, size / 2, degree * m + 1) for m in n]
    grids = np.meshgrid(*ax[::-1], indexing="ij")     # slowest first
    return np.stack([g.ravel() for g in grids[::-1]], axis=1)   # [node][x,y(,z)]


def csr_to_scipy(rp, col, val):
    import scipy.sparse as sp
    return sp.csr_matrix((val, col, rp), shape=(len(rp) - 1, len(rp) - 1))


def global_problem(mesh, deg):
    """global (unpartitioned) problem of the general-partition tests: mesh = "gmsh" (the bundled domain.msh) | "box:nx,ny[,nz]" | "refined:nx,ny[,nz]" (the box with its
    middle block [n/4, 3n/4) refined once: hanging nodes)"""
    if mesh == "gmsh":
        return pk.Problem.gmsh(DOMAIN_MSH, deg, material(), BC_2D)
    n = [int(v) for v in mesh.split(":")[1].split(",")]
    if mesh.startswith("refined:"):
        return pk.Problem.refined_box(len(n), n, [10.0] * len(n), deg, material(), BC_2D if len(n) == 2 else BC_3D, [m // 4 for m in n], [max(3 * m // 4, m // 4 + 1) for m in n])
    return box_problem(len(n), n, deg)


# ---- per-cell coefficient fields (test_permeability_cpu.py, test_moduli_cpu.py) ----------------------------------------------------------------------------------
ROLLERS3 = [(0, 0, 0.0), (2, 1, 0.0), (4, 2, 0.0)]


def centres(P):
    d = P.desc; nv = 1 << d.dim
    X = P.array("vertex_coords", (d.n_vertices, d.dim)); cv = P.array("cell_vertices", (d.n_cells, nv), np.int32)
    return X[cv].mean(axis=1)


def layered_field_problems():
    """a graded box of 3 x 2 x 5 cells and a refined box of 3 x 2 x 4 cells with three refined ones: the meshes the layers by cell centres are checked on"""
    mask = np.zeros(3 * 2 * 4, dtype=np.int32); mask[[1, 8, 23]] = 1
    return (pk.Problem.graded_box(3, [3, 2, 5], [3.0, 2.0, 4.0], 1, material(), ROLLERS3, [0.6, 0.0, 0.9]),
            pk.Problem.refined_box_mask(3, [3, 2, 4], [3.0, 2.0, 4.0], 1, material(), ROLLERS3, mask))


def refine_and_coarsen_pair():
    """(A, B, nc): two refined boxes over the same 3 x 2 x 4 = nc coarse cells; from A to B cell 1 is coarsened, 8 stays refined, 23 is refined"""
    n = [3, 2, 4]; nc = int(np.prod(n))

    def build(mask):
        return pk.Problem.refined_box_mask(3, n, [3.0, 2.0, 4.0], 1, material(), ROLLERS3, mask)
    m1 = np.zeros(nc, dtype=np.int32); m1[[1, 8]] = 1
    m2 = np.zeros(nc, dtype=np.int32); m2[[8, 23]] = 1
    return build(m1), build(m2), nc


def build_sanitized_check(tmp_path, name):
    """tests/<name>.cpp, a stand-alone program over a host-only header of csrc/ or host/, built with the address and undefined-behaviour sanitizers; returns the executable"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(root, "poroelasticity_dealii_amd", "csrc"),
                           os.path.join(root, "tests", name + ".cpp"), "-o", exe])
    return exe
