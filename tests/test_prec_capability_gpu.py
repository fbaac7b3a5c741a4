"""poro_supports_preconditioner() and the three solve entry points give the same answer for every (system, preconditioner) pair.

The host driver chooses its preconditioners from the query alone, so a pair the query accepts must solve, and a pair it refuses must be refused by the solve as well
(ctx_prec.hip: one verdict behind both).  Checked on one rank for every system (0 displacement, 1 pressure Jacobian, 2 projection) and every PREC_* value on tiny
contexts of each kind: boxes with the assembled and the matrix-free operator, a Gmsh grid, a refined box (hanging nodes, coarse space), a box with a drained face and
the same box with one node of the face left out of the list.

One asymmetry is known and kept: the query refuses PREC_CHEBYSHEV on the two Q1 systems, yet where no other refusal applies their solves run, and the test asserts
that they take PREC_JACOBI's iteration count - except on the pairs of CHEBYSHEV_NOT_AS_JACOBI, where the code before the verdict existed did not either (below)."""
import numpy as np
import pytest

import poroelasticity_dealii_amd as pk
from common import BC_2D, DOMAIN_MSH, box_problem, global_problem, material

pytestmark = pytest.mark.gpu
DT = 60.0
PRECS = (pk.PREC_NONE, pk.PREC_JACOBI, pk.PREC_SSOR, pk.PREC_FDM, pk.PREC_ILU0, pk.PREC_CHEBYSHEV, pk.PREC_TWO_LEVEL)
assert PRECS == tuple(range(7))


def drained(partial):
    """the box((2, 3, 5), [(5, 0.0)]) of test_pressure_bc_fdm_gpu.py; partial: one node of the face left out of the list (not a union of whole faces any more)"""
    P = pk.Problem.box(3, [2, 3, 5], [2.0, 3.0, 5.0], 1, material(), [(2 * d, d, 0.0) for d in range(3)]).set_pressure_bc([(5, 0.0)])
    if partial:
        P.desc.n_dirichlet_p -= 1
    return P


CONTEXTS = {
    "box-csr": (lambda: box_problem(2, 4, 2), pk.OP_CSR),
    "box-mf": (lambda: box_problem(2, 4, 2), pk.OP_MATRIX_FREE),
    "box3-mf": (lambda: box_problem(3, 3, 1), pk.OP_MATRIX_FREE),
    "gmsh": (lambda: pk.Problem.gmsh(DOMAIN_MSH, 1, material(), BC_2D), pk.OP_CSR),
    "refined": (lambda: global_problem("refined:8,8", 2), pk.OP_MATRIX_FREE),
    "drained-face": (lambda: drained(False), pk.OP_MATRIX_FREE),
    "drained-partial": (lambda: drained(True), pk.OP_MATRIX_FREE),
}

# Chebyshev on a Q1 system where another refusal comes first (constraint lists; prescribed pressures on system 1): refused like every other value.  Everywhere else the
# solve runs it (the asymmetry above)
CHEBYSHEV_Q1_REFUSED = {("refined", 1), ("refined", 2), ("drained-face", 1), ("drained-partial", 1)}

# (context, system, prec) where query and solve disagreed in the code before the verdict existed, beyond the asymmetry above: none
DISAGREEMENTS = set()

# A finding of the first run of this test, on the code before the verdict existed: Chebyshev on a Q1 system does not run as Jacobi but as PREC_NONE - the Krylov driver
# applies the diagonal for PREC_JACOBI alone, so a value without a form of its own on these systems is CG without a preconditioner.  The solve behaviour is kept (making
# it Jacobi, or an error, changes what runs); on these pairs the counts differ and the test asserts PREC_NONE's count instead.  Chebyshev / NONE / Jacobi iterations,
# identical before and after the verdict:
CHEBYSHEV_NOT_AS_JACOBI = {
    ("box-csr", 1): (14, 14, 10), ("box-mf", 1): (14, 14, 10),              # (their projection systems: 15 / 15 / 15, asserted as Jacobi)
    ("box3-mf", 1): (20, 20, 12), ("box3-mf", 2): (22, 22, 15),
    ("gmsh", 1): (30, 30, 24), ("gmsh", 2): (30, 30, 25),
    ("drained-face", 2): (40, 40, 22), ("drained-partial", 2): (40, 40, 22),
}


def assemble(G, system):
    """what the solve of `system` needs, from the same state every time, with a zero start vector"""
    if system == 0:
        G.set(pk.VEC_P, 1e6 * (1 + 0.1 * np.sin(0.37 * np.arange(G.n_p))))
        G.fill(pk.VEC_U, 0.0)
        G.disp_assemble_system()
    elif system == 1:
        p = 1e5 * (1 + 0.1 * np.sin(0.37 * np.arange(G.n_p)))
        G.set(pk.VEC_P, p); G.pres_apply_boundary_values(); G.copy(pk.VEC_P_OLD, pk.VEC_P)
        G.set(pk.VEC_P, 1.01 * p); G.pres_apply_boundary_values()
        G.pres_assemble_residual(DT); G.pres_assemble_jacobian(DT)
        G.fill(pk.VEC_DP, 0.0)
    else:
        G.set(pk.VEC_U, 1e-5 * np.sin(0.05 * np.arange(G.n_u)))
        G.proj_assemble_matrix(); G.proj_assemble_rhs([0])
        G.fill(pk.VEC_STRAIN0, 0.0)


def solve(G, system, prec):
    kw = dict(abs_tol=0.0, rel_tol=1e-8, max_iter=20000, prec=prec)
    return G.disp_solve(**kw) if system == 0 else G.pres_solve(**kw) if system == 1 else G.proj_solve(0, **kw)


@pytest.mark.parametrize("cid", list(CONTEXTS), ids=str)
def test_query_and_solves_agree(cid):
    build, mode = CONTEXTS[cid]
    P = build()
    G = pk.Context(P, 0, mode)
    try:
        if cid == "refined":
            assert P.desc.coarse.enabled and P.desc.cons_p.n > 0
        for system in (0, 1, 2):
            its = {}
            for prec in PRECS:
                assert (cid, system, prec) not in DISAGREEMENTS
                supported = G.supports_preconditioner(system, prec)
                assemble(G, system)
                asymmetry = not supported and prec == pk.PREC_CHEBYSHEV and system != 0 and (cid, system) not in CHEBYSHEV_Q1_REFUSED
                if supported or asymmetry:
                    rc, info = solve(G, system, prec)
                    print(f"{cid} system {system} prec {prec}: supported {supported}, rc {rc}, {info.iterations} iterations, converged {info.converged}")
                    assert rc == 0 and info.converged == 1, (cid, system, prec)
                    its[prec] = info.iterations
                    if asymmetry:
                        same_as = pk.PREC_NONE if (cid, system) in CHEBYSHEV_NOT_AS_JACOBI else pk.PREC_JACOBI
                        assert info.iterations == its[same_as], (cid, system, its)
                else:
                    with pytest.raises(RuntimeError):
                        solve(G, system, prec)
                    print(f"{cid} system {system} prec {prec}: refused by the query and by the solve")
    finally:
        G.close(); P.close()
