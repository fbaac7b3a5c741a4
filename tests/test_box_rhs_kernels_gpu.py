"""The two uniform-box right-hand side kernels in their second forms (kernels_box.hip): k_box_rhs_u_v2 stores a workgroup's dofs contiguously through LDS and reads lift / neu
only where a per-line flag (16 dofs = 128 bytes) says they hold something; k_box_proj_rhs_v2 stages the displacement nodes under a 16 x 16 tile of pressure nodes in LDS,
u plane by u plane.  Both promise the bits of the first forms, which PORO_BOX_KERNELS=v1 (read per call) runs: VEC_RHS_U and every VEC_PROJ_RHS0 + e are compared bit for
bit (sign bits of zeros included) between the two, and against tests/box_reference.py within 1e-11 of the reference's max - the bound of test_box_reference_gpu.py.

Boxes: the smallest ones, mixed extents, and around the sizes at which the new kernels change path - 15 / 16 / 17 pressure nodes per direction (the 16 x 16 tile; a tile is
one z plane deep, so every 3D box has more planes than a tile), and 255 / 256 / 258 - 261 displacement nodes in all (a workgroup of k_box_rhs_u_v2 owns 256 consecutive
nodes; 257 is prime and no box has it)."""
import numpy as np
import pytest

import oracle_py
import poroelasticity_dealii_amd as pk
from box_reference import BoxReference
from common import BC_2D, BC_3D, REF, box_problem

pytestmark = pytest.mark.gpu

HOOK = "PORO_BOX_KERNELS"
SMALL = [(3, (1, 1, 1)), (3, (2, 1, 3)), (3, (5, 3, 2)), (2, (3, 2))]
TILE_P = [(3, (14, 2, 1)), (3, (15, 2, 1)), (3, (16, 2, 1)), (3, (2, 14, 1)), (3, (2, 15, 1)), (3, (2, 16, 2)), (2, (14, 15)), (2, (16, 14)), (2, (15, 16))]
# (dim, cells, degree) by node count: Q1 255 = 15 x 17, 256 = 16 x 16, 258 = 2 x 129; 255 = 3 x 5 x 17, 256 = 4 x 8 x 8, 258 = 2 x 3 x 43; Q2 255 = 3 x 85 and 3 x 5 x 17, 261 = 3 x 87
NODES_256 = [(2, (14, 16), 1), (2, (15, 15), 1), (2, (1, 128), 1), (3, (2, 4, 16), 1), (3, (3, 7, 7), 1), (3, (1, 2, 42), 1), (2, (1, 42), 2), (3, (1, 2, 8), 2), (2, (1, 43), 2)]
CASES = [(dim, n, deg) for dim, n in SMALL + TILE_P for deg in (1, 2)] + NODES_256


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def rel(a, b):
    m = np.abs(b).max()
    return float(np.abs(a - b).max() / m) if m > 0 else float(np.abs(a - b).max())


def pairs(dim):
    return [(a, b) for a in range(dim) for b in range(a, dim)]


def both_forms(monkeypatch, P, dim, p, u):
    """([rhs_u, proj rhs ...] by the second forms, the same by the first forms) on one context: the hook is read per call"""
    G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        G.proj_assemble_matrix()
        res = []
        for v1 in (True, False, True):          # (the first forms again at the end: the flags of the second form leave nothing behind)
            if v1:
                monkeypatch.setenv(HOOK, "v1")
            else:
                monkeypatch.delenv(HOOK, raising=False)
            G.set(pk.VEC_P, p); G.disp_assemble_system(True)
            out = [G.get(pk.VEC_RHS_U).copy()]
            G.set(pk.VEC_U, u)
            G.proj_assemble_rhs([a * dim + b for a, b in pairs(dim)])
            out += [G.get(pk.VEC_PROJ_RHS0 + e).copy() for e in range(len(pairs(dim)))]
            res.append(out)
        for x, y in zip(res[0], res[2]):
            assert np.array_equal(bits(x), bits(y))
        return res[1], res[0]
    finally:
        monkeypatch.delenv(HOOK, raising=False)
        G.close()


def fields(P):
    n_p, n_u = P.desc.n_dofs_p, P.desc.n_dofs_u
    return REF["p_init"] * (1 + 0.3 * np.sin(0.37 * np.arange(n_p))), 1e-5 * np.sin(0.37 * np.arange(n_u)) + 1e-6 * np.cos(0.05 * np.arange(n_u))


def check(monkeypatch, dim, n, deg, bc=None, reference=True):
    P = box_problem(dim, n, deg, bc=bc)
    try:
        p, u = fields(P)
        new, old = both_forms(monkeypatch, P, dim, p, u)
        for k, (x, y) in enumerate(zip(new, old)):
            assert np.array_equal(bits(x), bits(y)), (k, int((bits(x) != bits(y)).sum()), float(np.abs(x - y).max()))
        if reference:
            R = BoxReference(P)
            errs = [rel(new[0], R.rhs_u(p))] + [rel(new[1 + k], R.proj_rhs(u, a, b)) for k, (a, b) in enumerate(pairs(dim))]
            print(f"{dim}D cells {n} Q{deg}: against the Kronecker reference rhs_u {errs[0]:.2e}, projection {max(errs[1:]):.2e}")
            assert max(errs) <= 1e-11, errs
        return new
    finally:
        P.close()


@pytest.mark.parametrize("dim,n,deg", CASES, ids=str)
def test_second_forms_give_the_bits_of_the_first(monkeypatch, dim, n, deg):
    """the bench's Dirichlet data: nonzero on one face of each pair, so lift is nonzero next to those faces and zero elsewhere"""
    check(monkeypatch, dim, n, deg)


@pytest.mark.parametrize("dim,n,deg", [(3, (5, 3, 2), 2), (3, (16, 2, 1), 1), (2, (15, 16), 2)], ids=str)
def test_lift_and_neu_zero_everywhere(monkeypatch, dim, n, deg):
    """homogeneous Dirichlet data and no load: no line of lift or neu is flagged, literal zeros stand in for all of them"""
    base = BC_3D if dim == 3 else BC_2D
    check(monkeypatch, dim, n, deg, bc=[(label, c, 0.0) for label, c, _ in base])


@pytest.mark.parametrize("dim,n,deg", [(2, (6, 6), 2), (3, (3, 3, 3), 1), (3, (16, 2, 1), 2)], ids=str)
def test_with_a_neumann_load(monkeypatch, dim, n, deg):
    """tractions on the high faces instead of displacements (as test_parity_gpu.test_neumann_traction): neu is nonzero on those faces.  The Kronecker reference has no
    traction term, so the right-hand side is checked against the CPU oracle here, with the same bound"""
    bc = [(0, 0, 0.0), (2, 1, 0.0)] + ([(4, 2, 0.0)] if dim == 3 else [])
    nm = [(1, 0, -2e6), (3, 1, -1e6)] + ([(5, 2, -3e6)] if dim == 3 else [])
    P = box_problem(dim, n, deg, bc=bc, neumann=nm)
    P0 = box_problem(dim, n, deg, bc=bc)
    try:
        p, u = fields(P)
        new, old = both_forms(monkeypatch, P, dim, p, u)
        for x, y in zip(new, old):
            assert np.array_equal(bits(x), bits(y))
        unloaded, _ = both_forms(monkeypatch, P0, dim, p, u)
        assert not np.array_equal(new[0], unloaded[0])                   # the load is in the right-hand side
        O = oracle_py.Oracle(P, hoisted=True)
        try:
            O.set(pk.VEC_P, p); O.disp_assemble_system(True)
            assert (e := rel(new[0], O.get(pk.VEC_RHS_U))) <= 1e-11, e
        finally:
            O.close()
    finally:
        P.close(); P0.close()


def test_signs_of_zeros(monkeypatch):
    """Displacements and pressures of the smallest subnormal size, negative: every product with a weight underflows to a signed zero.  The projection sums then hold -0.0
    wherever all the weights they meet are positive, and both forms give the same sign bits; the displacement right-hand side ends in `+ lift` with lift = +0.0 or a
    nonzero value, so none of its zeros is negative - in either form, also where literal zeros stand in for lift and neu"""
    tiny = np.float64(-5e-324)
    for dim, n, deg in ((3, (5, 3, 2), 2), (2, (15, 16), 1)):
        P = box_problem(dim, n, deg)
        try:
            new, old = both_forms(monkeypatch, P, dim, np.full(P.desc.n_dofs_p, tiny), np.full(P.desc.n_dofs_u, tiny))
            for x, y in zip(new, old):
                assert np.array_equal(bits(x), bits(y))
            assert not np.signbit(new[0][new[0] == 0]).any()
            negative_zeros = sum(int((np.signbit(x) & (x == 0)).sum()) for x in old[1:])
            print(f"{dim}D cells {n} Q{deg}: {negative_zeros} negative zeros in the projection right-hand sides")
            assert negative_zeros > 0
        finally:
            P.close()
