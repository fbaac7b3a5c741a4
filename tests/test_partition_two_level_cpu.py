"""The coarse space of PREC_TWO_LEVEL on the pieces of a general partition (Problem.partition(rank, n_ranks, coarse=True)): every piece carries its own copy of the
whole box problem and, for each local node, the global interpolation row of its global node; displacement ghosts and owners follow whole nodes, so the local numbering
stays node-interleaved even where the refined block touches a Dirichlet face.  Host provider only (no GPU)."""
import ctypes as C

import numpy as np
import pytest

import poroelasticity_dealii_amd as pk
from common import global_problem
from test_constraints_cpu import refined

# (name, builder, degree, ranks): the general-partition meshes, and the two refined boxes whose block touches a Dirichlet face (per-dof ghosting splits master nodes there)
CASES = [("refined:4,4,4", 2, 3), ("refined:6,5", 1, 3), ("gmsh", 2, 3), ("dirichlet_3d", 2, 3), ("dirichlet_2d", 1, 2)]


def build(name, deg):
    if name == "dirichlet_3d":
        return refined(3, (3, 3, 2), deg, (1, 1, 0), (2, 2, 1))
    if name == "dirichlet_2d":
        return refined(2, (3, 3), deg, (0, 0), (2, 1))
    return global_problem(name, deg)


def arr(ptr, n, dtype=None):
    return np.ctypeslib.as_array(ptr, shape=(int(n),)).copy() if n else np.zeros(0, dtype or np.float64)


def rows(cs, n_rows, pressure=False):
    """(ptr, node, weight) of the displacement (per node) or pressure interpolation"""
    p = arr(cs.ptr_p if pressure else cs.ptr, n_rows + 1)
    return p, arr(cs.node_p if pressure else cs.node, p[-1], np.int32), arr(cs.weight_p if pressure else cs.weight, p[-1])


def box_desc(d):
    return C.cast(d.coarse.box_problem, C.POINTER(pk.Desc)).contents


def restrict(ptr, node, w, n_coarse, vals, ncomp):
    """P^T v over the given rows: vals[row, comp]"""
    nnz = int(ptr[-1]); row = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    out = np.zeros((n_coarse, ncomp))
    np.add.at(out, node[:nnz], w[:nnz, None] * vals[row])
    return out


@pytest.mark.parametrize("name,deg,world", CASES)
def test_pieces_carry_the_coarse_space(name, deg, world):
    PG = build(name, deg)
    pieces = [PG.partition(r, world, coarse=True) for r in range(world)]
    try:
        dG = PG.desc; dim = dG.dim
        assert dG.coarse.enabled
        bG = box_desc(dG)
        gp, gn, gw = rows(dG.coarse, dG.n_dofs_u // dim)
        gpp, gnp, gwp = rows(dG.coarse, dG.n_dofs_p, pressure=True)
        nH, nHp = bG.n_dofs_u // dim, bG.n_dofs_p
        rng = np.random.default_rng(7)
        gu = rng.standard_normal(dG.n_dofs_u); gpres = rng.standard_normal(dG.n_dofs_p)
        ref_u = restrict(gp, gn, gw, nH, gu.reshape(-1, dim), dim); ref_p = restrict(gpp, gnp, gwp, nHp, gpres[:, None], 1)
        sum_u = np.zeros_like(ref_u); sum_p = np.zeros_like(ref_p)
        gdir = dict(zip(arr(bG.dirichlet_dof, bG.n_dirichlet, np.int32).tolist(), arr(bG.dirichlet_value, bG.n_dirichlet).tolist()))
        for P in pieces:
            d = P.desc; pt = d.part; l2g = P.local_to_global_u; l2gp = P.local_to_global_p
            assert d.coarse.enabled == 1 and pt.n_neighbours > 0
            # the box problem equals the global one: sizes, box tag, Dirichlet list
            b = box_desc(d)
            assert (b.dim, b.degree_u, b.n_cells, b.n_dofs_u, b.n_dofs_p) == (bG.dim, bG.degree_u, bG.n_cells, bG.n_dofs_u, bG.n_dofs_p)
            assert b.box.enabled == 1 and list(b.box.n) == list(bG.box.n) and list(b.box.h) == list(bG.box.h) and list(b.box.origin) == list(bG.box.origin)
            assert b.part.n_ranks == 1 and b.part.n_neighbours == 0 and not b.coarse.enabled
            assert dict(zip(arr(b.dirichlet_dof, b.n_dirichlet, np.int32).tolist(), arr(b.dirichlet_value, b.n_dirichlet).tolist())) == gdir
            # node-interleaved local numbering, ghosts included; owned nodes first
            assert pt.n_owned_u % dim == 0 and d.n_dofs_u % dim == 0
            nodes = l2g.reshape(-1, dim)
            assert np.all(nodes[:, 0] % dim == 0) and all(np.array_equal(nodes[:, c], nodes[:, 0] + c) for c in range(dim))
            # each local node's row is the global row of its global node (same entries, same order)
            p, n, w = rows(d.coarse, d.n_dofs_u // dim)
            for i, g in enumerate(nodes[:, 0] // dim):
                assert np.array_equal(n[p[i]:p[i + 1]], gn[gp[g]:gp[g + 1]]) and np.array_equal(w[p[i]:p[i + 1]], gw[gp[g]:gp[g + 1]])
            pp, nq, wq = rows(d.coarse, d.n_dofs_p, pressure=True)
            for i, g in enumerate(l2gp):
                assert np.array_equal(nq[pp[i]:pp[i + 1]], gnp[gpp[g]:gpp[g + 1]]) and np.array_equal(wq[pp[i]:pp[i + 1]], gwp[gpp[g]:gpp[g + 1]])
            # every master of a local constrained dof is local
            if d.cons_u.n:
                cp = arr(d.cons_u.ptr, d.cons_u.n + 1); m = arr(d.cons_u.master, cp[-1], np.int32); dof = arr(d.cons_u.dof, d.cons_u.n, np.int32)
                assert m.min() >= 0 and m.max() < d.n_dofs_u and not set(m.tolist()) & set(dof.tolist())
            # owned-row restrictions
            own = pt.n_owned_u // dim
            sum_u += restrict(p[:own + 1], n, w, nH, gu[l2g].reshape(-1, dim)[:own], dim)
            sum_p += restrict(pp[:pt.n_owned_p + 1], nq, wq, nHp, gpres[l2gp][:pt.n_owned_p, None], 1)
        assert np.linalg.norm(sum_u - ref_u) <= 1e-14 * np.linalg.norm(ref_u)
        assert np.linalg.norm(sum_p - ref_p) <= 1e-14 * np.linalg.norm(ref_p)
        assert sum(P.desc.part.n_owned_u for P in pieces) == dG.n_dofs_u and sum(P.desc.part.n_owned_p for P in pieces) == dG.n_dofs_p
        # the pieces' box copies outlive the global problem
        PG.close()
        for P in pieces:
            b = box_desc(P.desc)
            assert b.box.enabled == 1 and b.n_dofs_u == nH * dim
            assert dict(zip(arr(b.dirichlet_dof, b.n_dirichlet, np.int32).tolist(), arr(b.dirichlet_value, b.n_dirichlet).tolist())) == gdir
    finally:
        for P in pieces:
            P.close()
        PG.close()


def test_pieces_without_the_flag_have_no_coarse_space():
    PG = global_problem("refined:4,4,4", 2)
    try:
        assert PG.desc.coarse.enabled
        for r in range(3):
            P = PG.partition(r, 3)
            assert P.desc.coarse.enabled == 0
            P.close()
    finally:
        PG.close()


def test_the_flag_needs_a_coarse_space():
    PG = global_problem("box:4,4", 1)
    try:
        assert not PG.desc.coarse.enabled
        with pytest.raises(RuntimeError, match="coarse space"):
            PG.partition(0, 2, coarse=True)
    finally:
        PG.close()
