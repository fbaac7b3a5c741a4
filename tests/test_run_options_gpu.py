"""The run options from the keyword arguments of run_problem / Runner to the contexts the host driver creates (RunOptions -> poro_host_run_options -> RunControls,
host/run_controls.hpp): every switch is read back from the context it was meant for, also from the context of an adapted mesh, and a Chebyshev run with an explicit
degree and interval ratio repeats the trace recorded on the commit before the options struct (tests/golden/run_options_cheb_trace.npy), bit for bit."""
import os

import numpy as np
import pytest

import poroelasticity_dealii_amd as pk
from common import BC_3D, GOLDEN, REF, box_problem, host_material
from hybrid_reference import make_mask

pytestmark = pytest.mark.gpu


def readings(R):
    return (R.ctx.get_fdm_precision()[0], R.ctx.get_fdm_form()[0], R.ctx.get_moduli_operator()[0], R.ctx.get_scatter_mode(), R.preconditioners())


def test_every_switch_reaches_the_context_of_a_runner():
    """4^3 Q2 box, Dirichlet data on both faces of every direction.  A plain box carries no coarse space, so with two_level_p the projection solve of initialize() is
    refused - after the requests went to the context and the preconditioners were chosen, which is what is read back.  The scatter mode: the structured kernels of a
    constant-coefficient box have no scatter and poro_ctx_set_scatter_mode records nothing there (as on every commit before), so the request is read back from the same
    box with moduli layered along z, which runs the general cell loop"""
    on = dict(prec=pk.PREC_FDM, fdm_fp32=True, fdm_per_direction=True, moduli_structured=True, atomic_scatter=True, reduction=True, two_level_p=True)
    P = box_problem(3, 4, 2, mat=host_material(), bc=BC_3D)
    try:
        for layered, scatter in ((False, pk.SCATTER_COLOURED), (True, pk.SCATTER_ATOMIC)):
            if layered:
                P.set_moduli_layers([(0.0, REF["E"], REF["nu"]), (5.0, 2.0 * REF["E"], REF["nu"])])
            R = pk.Runner(P, 0, pk.OP_MATRIX_FREE, p_init=REF["p_init"], dt=REF["dt"], **on)
            try:
                with pytest.raises(RuntimeError, match="PORO_PREC_TWO_LEVEL"):
                    R.initialize()
                assert readings(R) == (pk.FDM_FP32, pk.FDM_FORM_PER_DIRECTION, pk.MODULI_OP_STRUCTURED, scatter, (pk.PREC_FDM, pk.PREC_TWO_LEVEL, pk.PREC_TWO_LEVEL))
            finally:
                R.close()
        P.set_cell_moduli(None, None)
        R = pk.Runner(P, 0, pk.OP_MATRIX_FREE, p_init=REF["p_init"], dt=REF["dt"], prec=pk.PREC_FDM)      # every switch off
        try:
            R.initialize()
            # (pressure and projection: the strongest form a box supports)
            assert readings(R) == (pk.FDM_FP64, pk.FDM_FORM_DEFAULT, pk.MODULI_OP_CELLS, pk.SCATTER_COLOURED, (pk.PREC_FDM, pk.PREC_FDM, pk.PREC_FDM))
        finally:
            R.close()
    finally:
        P.close()


def test_the_requests_follow_an_adaptive_run_to_its_last_mesh():
    """2 x 2 x 2 Q2 box with its corner cell refined, adapted before both steps: the context the run ends on belongs to a mesh the run built and still reports both requests"""
    P = pk.Problem.refined_box_mask(3, [2, 2, 2], [10.0] * 3, 2, host_material(), BC_3D, make_mask("corner", (2, 2, 2)))
    try:
        trace, G = pk.run_problem(P, 2, REF["p_init"], REF["dt"], operator_mode=pk.OP_MATRIX_FREE, prec=-1, refine_every=1, hybrid_operator=True, fdm_per_direction=True)
        last = G.problem
        try:
            assert last is not P and int(trace[-1, 0]) == 2
            assert G.get_operator_form()[0] == pk.OPFORM_HYBRID
            assert G.get_fdm_form()[0] == pk.FDM_FORM_PER_DIRECTION
        finally:
            G.close(); last.close()
    finally:
        P.close()


def test_chebyshev_degree_and_ratio_repeat_the_recorded_trace():
    P = box_problem(3, 4, 2, mat=host_material())
    try:
        trace, G = pk.run_problem(P, 1, REF["p_init"], REF["dt"], device=0, operator_mode=pk.OP_MATRIX_FREE, max_it=5000, prec=pk.PREC_CHEBYSHEV, cheb_degree=2, cheb_ratio=30)
        G.close()
        want = np.load(os.path.join(GOLDEN, "run_options_cheb_trace.npy"))
        assert trace.shape == want.shape and trace.tobytes() == want.tobytes(), (trace, want)
    finally:
        P.close()
