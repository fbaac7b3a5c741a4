"""General partitions with the atomic scatter mode of the matrix-free operator (PORO_MFG_SCATTER=atomic, inherited by the rank processes): every rank's
partial product comes from the single atomic launch, then goes through the same pack -> exchange -> ordered-sum sequence.  The helper's checks hold
unchanged, among them the bitwise equality of the shared copies across ranks: the interface sums are rank-ordered whatever produced the partials."""
import numpy as np
import pytest

import poroelasticity_dealii_amd as pk
from common import global_problem
from test_partition_general_cpu import check_against_single_rank, run_ranks

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("world,mesh,deg,backend", [(3, "gmsh", 2, "hip_mf"), (4, "box:4,4,4", 2, "hip_mf"), (3, "refined:4,4,4", 2, "hip_mf"), (2, "box:7,6", 2, "hip_mf_cheb")])
def test_general_partition_with_atomic_scatter(tmp_path, monkeypatch, world, mesh, deg, backend):
    monkeypatch.setenv("PORO_MFG_SCATTER", "atomic")
    # the switch is in force for contexts created in this environment, which run_ranks hands to the rank processes: a context on a general mesh starts in the atomic
    # mode and makes one cell-kernel launch per application
    P = global_problem("gmsh", deg)
    G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        assert G.get_scatter_mode() == pk.SCATTER_ATOMIC
        G.fill(pk.VEC_P, 0.0); G.disp_assemble_system(True)
        G.timers_reset(); G.apply(pk.MAT_A_U, np.ones(G.n_u))
        assert G.timer("mfg_cell_kernels")[1] == 1
    finally:
        G.close(); P.close()
    R = run_ranks(tmp_path, world, mesh, deg, backend)
    check_against_single_rank(R, mesh, deg, tol_u=1e-8)
