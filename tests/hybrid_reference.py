"""Helpers of the hybrid-operator tests (poro_ctx_set_operator_form, PORO_OPFORM_HYBRID), not collected: the shapes and masks of the issue, the plan of the hybrid form
restated in NumPy from Problem.cell_parents() and the interpolation rows of poro_desc.coarse, and the identity

    A x = S (A_box x_box - sum_{refined box cells c} K_c x_box) + sum_{fine cells f} K_f x,      x_box = S^T x

evaluated with tests/general_reference.py's GeneralReference (S = the injection box node -> mesh node)."""
import copy
import ctypes as C

import numpy as np

import poroelasticity_dealii_amd as pk
from common import BC_2D, BC_3D, material
from general_reference import GeneralReference

# box sizes per (dim, degree): they cross the tile edges of the structured kernels, give two z-chunks and ragged last workgroups of the cell kernels
SHAPES = [(3, 2, (4, 4, 4)), (3, 2, (3, 5, 7)), (3, 1, (4, 4, 4)), (3, 1, (3, 3, 7)), (2, 2, (8, 8)), (2, 2, (5, 13)), (2, 1, (8, 8)), (2, 1, (7, 9))]
MASKS = ["none", "all", "block", "corner", "random"]


def shape_id(dim, deg, n):
    return f"{dim}d-q{deg}-{'x'.join(map(str, n))}"


def make_mask(name, n):
    """one int32 per coarse cell, x fastest"""
    m = np.zeros(tuple(n)[::-1], dtype=np.int32)          # [z][y][x]
    if name == "all":
        m[...] = 1
    elif name == "block":                                  # [1, n - 1) in every direction
        m[tuple(slice(1, k - 1) for k in tuple(n)[::-1])] = 1
    elif name == "corner":                                 # the cell in the corner of the faces 0, 2 (, 4): all of them carry Dirichlet data
        m[(0,) * len(n)] = 1
    elif name == "random":                                 # fixed seed, 30 %
        m = (np.random.default_rng(12345).random(m.shape) < 0.3).astype(np.int32)
    elif name != "none":
        raise ValueError(name)
    return m.reshape(-1)


def refined_problem(dim, deg, n, mask):
    return pk.Problem.refined_box_mask(dim, list(n), [10.0] * dim, deg, material(), BC_2D if dim == 2 else BC_3D, mask)


class CoarseBox:
    """the uniform box a refined box carries as poro_desc.coarse.box_problem, as a problem GeneralReference accepts (the refined problem keeps it alive)"""

    def __init__(self, problem):
        assert problem.desc.coarse.enabled
        self.owner = problem
        self.desc_ptr = C.cast(problem.desc.coarse.box_problem, C.POINTER(pk.Desc))
        self.desc = self.desc_ptr.contents


def interpolation_rows(problem):
    d = problem.desc
    nn = d.n_dofs_u // d.dim
    ptr = np.ctypeslib.as_array(d.coarse.ptr, shape=(nn + 1,)).copy()
    node = np.ctypeslib.as_array(d.coarse.node, shape=(int(ptr[-1]),)).copy()
    w = np.ctypeslib.as_array(d.coarse.weight, shape=(int(ptr[-1]),)).copy()
    return ptr, node, w


class HybridPlan:
    """inj [box node] -> mesh node (the mesh node whose interpolation row is the single entry (b, 1.0)); unrefined: mesh cells with a box twin, twin: their box cells;
    removed: the refined box cells; fine: their children among the mesh cells.  The cell classes come from cell_parents()"""

    def __init__(self, problem):
        d = problem.desc
        self.dim = dim = d.dim
        box = CoarseBox(problem).desc
        nb = box.n_dofs_u // dim
        ptr, node, w = interpolation_rows(problem)
        single = np.where((np.diff(ptr) == 1) & (w[np.minimum(ptr[:-1], len(w) - 1)] == 1.0))[0]
        self.inj = np.full(nb, -1, dtype=np.int64)
        self.inj[node[ptr[single]]] = single
        assert (self.inj >= 0).all() and len(single) == nb, "every box node has exactly one injected image"
        self.inj_dofs = (self.inj[:, None] * dim + np.arange(dim)[None, :]).reshape(-1)      # [box dof] -> mesh dof
        coarse, child = problem.cell_parents()
        self.unrefined = np.where(child < 0)[0]
        self.twin = coarse[self.unrefined]
        self.fine = np.where(child >= 0)[0]
        self.removed = np.unique(coarse[self.fine])
        self.mask = problem.refine_mask()
        assert np.array_equal(np.where(self.mask != 0)[0], self.removed)
        assert len(self.fine) == len(self.removed) << dim
        assert np.array_equal(np.sort(np.concatenate([self.twin, self.removed])), np.arange(box.n_cells))


def restricted(R, cells):
    """the reference over a subset of its cells"""
    S = copy.copy(R)
    S.cv, S.cdu, S.n_cells = R.cv[cells], R.cdu[cells], len(cells)
    return S


class HybridReference:
    """the right-hand side of the identity, term by term with GeneralReference"""

    def __init__(self, problem, R=None):
        self.plan = plan = HybridPlan(problem)
        self.R = R or GeneralReference(problem)
        self.Rbox = GeneralReference(CoarseBox(problem))
        self.fine, self.gone = restricted(self.R, plan.fine), restricted(self.Rbox, plan.removed)
        # what the library matches cells by: the dof list of an unrefined cell is, entry by entry, the injected dof list of its box cell; same Dirichlet mask
        assert np.array_equal(self.R.cdu[plan.unrefined], plan.inj_dofs[self.Rbox.cdu[plan.twin]])
        assert np.array_equal(self.R.mask[plan.inj_dofs], self.Rbox.mask)

    def apply_full(self, x):
        x = np.asarray(x, dtype=np.float64)
        xb = x[self.plan.inj_dofs]
        y = self.fine.apply_full(x)
        y[self.plan.inj_dofs] += self.Rbox.apply_full(xb) - self.gone.apply_full(xb)
        return y

    def apply_A(self, x):
        """the convention of GeneralReference.apply_A: constrained columns dropped, a Dirichlet row keeps its full diagonal"""
        x = np.asarray(x, dtype=np.float64)
        m = self.R.mask
        y = self.apply_full(np.where(m, 0.0, x))
        if m.any():
            y[m] = self.R.diag_full()[m] * x[m]
        return y


def spike_dofs(problem, plan, R):
    """mesh dofs for unit spikes: a box node interior to a refined region, an interface node (refined and unrefined cells around it), a hanging node, a Dirichlet
    dof and the last box node - those of them the mask has"""
    dim = plan.dim
    box = CoarseBox(problem).desc
    cdb = np.ctypeslib.as_array(box.cell_dofs_u, shape=(box.n_cells, R.dpc))[:, ::dim] // dim       # [box cell] -> its box nodes
    nb = box.n_dofs_u // dim
    around = np.bincount(cdb.reshape(-1), minlength=nb)
    gone = np.bincount(cdb[plan.removed].reshape(-1), minlength=nb)
    out = {}
    inner = np.where((gone == around) & (around == 1 << dim))[0]
    if len(inner):
        out["interior of a refined region"] = int(plan.inj[inner[len(inner) // 2]]) * dim
    rim = np.where((gone > 0) & (gone < around))[0]
    if len(rim):
        out["interface node"] = int(plan.inj[rim[len(rim) // 2]]) * dim + dim - 1
    nh = problem.desc.cons_u.n
    if nh:
        out["hanging node"] = int(np.ctypeslib.as_array(problem.desc.cons_u.dof, shape=(nh,))[nh // 2])
    out["Dirichlet dof"] = int(R.dir_dof[len(R.dir_dof) // 2])
    out["last box node"] = int(plan.inj[nb - 1]) * dim + dim - 1
    return out
