"""Prescribed pressures beside hanging pressure nodes (a drained face on a locally refined mesh), host side: the meshes the GPU tests use, what the host provider's two
lists look like on them, and that the coarse problem of the two-level preconditioner learns of a pressure condition set after it was built.

M2 / M3 are Terzaghi's column (tests/test_terzaghi.py) as a refined box whose layer below the drained top is refined together with ONE cell of the top layer: the hanging
node on the edge (2D) or face (3D) between two top cells then has prescribed masters.  Those are the rows on which a pressure that is only SET on the prescribed dofs
stays non-conforming."""
import numpy as np
import pytest

import poroelasticity_dealii_amd as pk
from common import BC_2D, DOMAIN_MSH, material
from test_constraints_cpu import cons_arrays

H, SIGMA0 = 10.0, 1.0e6


def column_bc(dim):
    last = dim - 1
    return [(2 * d, d, 0.0) for d in range(dim - 1)] + [(2 * d + 1, d, 0.0) for d in range(dim - 1)] + [(2 * last, last, 0.0)], [(2 * last + 1, last, -SIGMA0)]


def column_cells(dim):
    return [2, 10] if dim == 2 else [2, 2, 6]


def column_mask(dim, kind):
    """kind: "zero" | "one" | "top2" (the two top layers: hanging nodes between layers only) | "M" (M2 / M3: the layer below the top and one cell of the top layer)"""
    n = column_cells(dim); ny = n[-1]; per = 2 ** (dim - 1)
    mask = np.zeros(int(np.prod(n)), dtype=np.int32)
    if kind == "one":
        mask[:] = 1
    elif kind == "top2":
        mask[per * (ny - 2):] = 1
    elif kind == "M":
        mask[per * (ny - 2):per * (ny - 1)] = 1; mask[per * (ny - 1)] = 1
    else:
        assert kind == "zero"
    return mask


def drained_column(dim, deg, kind="M", value=0.0):
    """(problem, material): the column with a drained top on the mask `kind`"""
    m = material(flow_rate=0.0)
    bc, neu = column_bc(dim)
    P = pk.Problem.refined_box_mask(dim, column_cells(dim), [10.0] * (dim - 1) + [H], deg, m, bc, column_mask(dim, kind), neu)
    P.set_pressure_bc([(2 * (dim - 1) + 1, value)])
    return P, m


def prescribed(desc):
    n = desc.n_dirichlet_p
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0)
    return np.ctypeslib.as_array(desc.dirichlet_dof_p, shape=(n,)).copy(), np.ctypeslib.as_array(desc.dirichlet_value_p, shape=(n,)).copy()


def violation(P, p):
    """max over the constraint rows of |p[h] - sum w p[m] - b|"""
    dof, ptr, m, w, inh = cons_arrays(P.desc.cons_p)
    if len(dof) == 0:
        return 0.0
    return max(abs(p[dof[i]] - w[ptr[i]:ptr[i + 1]] @ p[m[ptr[i]:ptr[i + 1]]] - inh[i]) for i in range(len(dof)))


def coarse_desc(P):
    import ctypes as C
    assert P.desc.coarse.enabled and P.desc.coarse.box_problem
    return C.cast(P.desc.coarse.box_problem, C.POINTER(pk.Desc)).contents


@pytest.mark.parametrize("dim,cells,n_p,n_pdir,n_hang,rows_with_prescribed_master,in_both", [(2, 29, 46, 4, 4, 1, 0), (3, 59, 134, 14, 36, 7, 2)], ids=["M2", "M3"])
def test_lists_of_the_two_columns(dim, cells, n_p, n_pdir, n_hang, rows_with_prescribed_master, in_both):
    P, _ = drained_column(dim, 1)
    try:
        d = P.desc
        pd, pv = prescribed(d)
        dof, ptr, m, w, inh = cons_arrays(d.cons_p)
        assert (d.n_cells, d.n_dofs_p, len(pd), len(dof)) == (cells, n_p, n_pdir, n_hang)
        is_pd = np.zeros(d.n_dofs_p, bool); is_pd[pd] = True
        with_master = [i for i in range(len(dof)) if is_pd[m[ptr[i]:ptr[i + 1]]].any()]
        both = [i for i in range(len(dof)) if is_pd[dof[i]]]
        assert len(with_master) == rows_with_prescribed_master and len(both) == in_both
        for i in both:                                                   # the consistency rule of the library: all masters prescribed, the value is theirs
            assert is_pd[m[ptr[i]:ptr[i + 1]]].all()
        # a pressure that is only SET on the prescribed dofs of a constant field violates exactly the rows with a prescribed master that are not prescribed themselves, by half
        # (2D: one of two masters; 3D edge midpoints likewise) or more of the constant
        p = np.full(d.n_dofs_p, 1.0); p[pd] = pv
        bad = [i for i in range(len(dof)) if abs(p[dof[i]] - w[ptr[i]:ptr[i + 1]] @ p[m[ptr[i]:ptr[i + 1]]]) > 1e-14]
        assert sorted(bad) == sorted(set(with_master) - set(both)) and violation(P, p) >= 0.25
    finally:
        P.close()


def test_coarse_problem_of_a_refined_box_learns_of_the_condition():
    bc, neu = column_bc(2)
    P = pk.Problem.refined_box_mask(2, [4, 3], [10.0, H], 2, material(flow_rate=0.0), bc, [0, 0, 0, 0, 0, 1, 1, 0, 0, 1, 1, 0], neu)
    try:
        Hd = coarse_desc(P)
        assert Hd.n_dirichlet_p == 0 and P.desc.n_dirichlet_p == 0
        P.set_pressure_bc([(3, 2.5e5)])
        Hd = coarse_desc(P)
        pd, pv = prescribed(Hd)
        assert sorted(pd) == list(range(5 * 3, 5 * 4)) and np.all(pv == 2.5e5)         # the whole top line of the 4 x 3 box (lexicographic vertices)
        assert P.desc.n_dirichlet_p == 4 + 1 + 2                                       # 4 x 3 cells, the two middle top cells refined: 7 vertices on the top side
        P.set_pressure_bc([])                                                          # ... and of its removal
        assert coarse_desc(P).n_dirichlet_p == 0 and P.desc.n_dirichlet_p == 0
    finally:
        P.close()


def test_auxiliary_box_of_a_gmsh_grid_learns_of_the_condition():
    P = pk.Problem.gmsh(DOMAIN_MSH, 1, material(), BC_2D)
    try:
        d = P.desc
        assert d.coarse.enabled and coarse_desc(P).n_dirichlet_p == 0
        X = np.ctypeslib.as_array(d.vertex_coords, shape=(d.n_vertices, 2))
        ids = sorted(set(np.ctypeslib.as_array(d.bface_id, shape=(d.n_bfaces,))))
        for label in ids:                                                              # one id per side; the box numbers its sides by direction, Gmsh counter-clockwise
            P.set_pressure_bc([(int(label), 0.0)])
            pd, _ = prescribed(P.desc)
            Hd = coarse_desc(P)
            hd, _ = prescribed(Hd)
            XH = np.ctypeslib.as_array(Hd.vertex_coords, shape=(Hd.n_vertices, 2))
            assert len(pd) > 0 and len(hd) > 0
            # the same side of the rectangle: one coordinate is constant over both sets and equal, and the box lists EVERY vertex it has there
            k = int(np.argmin(np.ptp(X[pd], axis=0)))
            side = X[pd][0, k]
            assert np.ptp(X[pd][:, k]) <= 1e-9 and np.abs(XH[hd][:, k] - side).max() <= 1e-9
            assert len(hd) == int((np.abs(XH[:, k] - side) <= 1e-9).sum())
    finally:
        P.close()
