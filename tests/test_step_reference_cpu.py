"""The independent model of the time step (tests/step_reference.py) checks itself, without a GPU.

1. Constant coefficients, no gravity, the reference's boundary conditions: walk() in the default flavour reproduces the five cases of tests/golden/independent_traces.json
   (the Kronecker-product model of tools/independent_model.py) to the tolerances of tests/test_independent_golden.py.
2. On every case of tests/test_step_reference_gpu.py the coupled / incremental walk() converges to monolithic_step over two steps: d_ref (max norm, relative, of u, p and
   eps_v) < 1e-9 with fss_tol = pressure_tol = 1e-10 of the case's first residual, in at most 100 fixed-stress iterations per step.
3. Sensitivity: one ingredient of the reference changed by a relative 1e-3 moves u or p, after step 1 and after step 2, by at least 100 times the largest bound the GPU
   test uses for the case; so does reading the per-cell arrays in a transposed cell order.
4. Default flavour: every stopping decision of walk() is at least a factor 2 from its threshold, so the device must take the same iteration counts.

How the cases were chosen (tests/step_reference.py, Case): p_init = 1e5 Pa and not the 10 MPa of input.data, so that gravity (rho g L = 2.5e5 Pa) and not the initial
pressure carries the displacement - a cell's density then moves u by 5e-5 and more; the prescribed pressures far from p_init (0.1 and 0.2 p_init), so that the drained
face drives flow across several cells within two steps and a layer's permeability and the storage term move p by 5e-6 and more; the modulus fields of the boxes, the
graded and the refined meshes (the default-flavour cases among them) >= 3 times the material's, so that the inner pressure iteration contracts by
alpha^2 M_b / K_node <= 0.12 per pass and two consecutive residuals lie a factor > 8 apart - room for a tolerance a factor 3 from both - while the jittered meshes keep the
material's scale (a stronger coupling: the storage term moves p by 1.2e-5 and not 4e-6); the stiffer layer of box3_q2 on top (a layer ten times SOFTER than the
material makes that iteration diverge).  In box3_q2 the top face carries the traction and therefore no condition on u_z: with all of BC_3D no normal traction acts on
any free dof.  jitter3_q2 has a drained top: as a closed box it hardly flows.

Measured (this file's output):
  case                 cells  dofs u + p   fixed-stress its   d_ref (largest of u, p, eps_v over both steps)   weakest perturbation, in bounds on u and p
  box3_q2              24     945 + 60     6, 6               6.5e-11                                           alpha in the storage term       446 x 1e-8
  box2_q1              20     60 + 30      6, 6               3.0e-10                                           alpha in the storage term      5711 x 1e-8
  graded3_q2           27     1029 + 64    6, 6               4.9e-11                                           alpha in the storage term       267 x 1e-7
  refined3_q1          46     315 + 105    5, 5               5.0e-11                                           alpha in the storage term       126 x 1e-7
  refined3_q2          46     1725 + 105   5, 5               2.6e-11                                           alpha in the storage term       131 x 1e-7
  refined3_q2_hybrid   46     1725 + 105   7, 7               8.1e-11                                           kappa_x of the lower layer      403 x 1e-7
  jitter2_q2           16     162 + 25     9, 9               2.0e-10                                           lambda of the lower layer       474 x 1e-7
  jitter3_q2           27     1029 + 64    6, 6               3.6e-11                                           alpha in the storage term       117 x 1e-7
Every other perturbation moves u or p by 400 to 3e5 bounds, the transposed cell arrays by 1e6 and more (-s prints every row).  |Du - S| / |Du| <= 1.7e-15 on every case but
jitter3_q2 (1.8e-2).  Default flavour: box3_q2 tolerance 7.5e-9 of the first residual, rows (1, 7), (1, 7), closest decision a factor 3.12 from its threshold;
refined3_q2 3.2e-7, (1, 5), (1, 5), 3.58; box2_q1 7.5e-9, (1, 7), (1, 7), 3.77.  The five goldens: counts equal, |p|_inf to 6e-16, fields to 5e-14."""
import json
import os

import numpy as np
import pytest

from common import GOLDEN, REF, box_problem
from step_reference import CASES, COUPLED_REL, DEFAULT_REL, DT, Case, StepReference, case_bound, distance

with open(os.path.join(GOLDEN, "independent_traces.json")) as f:
    GOLD = json.load(f)


@pytest.mark.parametrize("key", sorted(GOLD))
def test_walk_reproduces_the_kronecker_model(key):
    g = GOLD[key]
    P = box_problem(g["dim"], g["n"], g["degree"])
    try:
        W = StepReference(P, REF["dt"], REF["p_init"]).walk(g["steps"], 1e-8, 1e-8)
        tr = W["trace"]
        u, p = W["states"][-1][:2]
        assert [t[2] for t in tr] == [t["pressure_iterations"] for t in g["trace"]]
        assert [t[1] for t in tr] == [t["fss_iteration"] for t in g["trace"]]
        for r, t in zip(tr, g["trace"]):
            assert abs(r[3] - t["p_linf"]) <= 1e-10 * t["p_linf"]
        assert abs(np.linalg.norm(u) - g["u_l2"]) <= 1e-8 * g["u_l2"] and abs(np.linalg.norm(p) - g["p_l2"]) <= 1e-11 * g["p_l2"]
        up, pp = u[:: max(1, len(u) // 16)][:16], p[:: max(1, len(p) // 16)][:16]
        assert np.abs(up - np.array(g["u_probe"])).max() <= 1e-8 * np.abs(u).max()
        assert np.abs(pp - np.array(g["p_probe"])).max() <= 1e-11 * np.abs(p).max()
    finally:
        P.close()


@pytest.fixture(scope="module")
def shared(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("step_reference")
    made = {}

    def get(name):
        if name not in made:
            C = Case(name, tmp)
            R = C.reference()
            s0 = R.initial_state()
            m1 = R.monolithic_step(s0[0], s0[1])
            made[name] = (C, R, (s0, m1, R.monolithic_step(m1[0], m1[1])))
        return made[name]
    yield get
    for C, _, _ in made.values():
        C.close()


@pytest.mark.parametrize("name", list(CASES), ids=str)
def test_coupled_loop_converges_to_the_monolithic_step(shared, name):
    C, R, (s0, m1, m2) = shared(name)
    tol = COUPLED_REL * R.first_residual()
    W = R.walk(2, tol, tol, max_fss=200, coupled=True, incremental=True)
    its = [sum(1 for t in W["trace"] if t[0] == s) for s in (1, 2)]
    d1, d2 = distance(W["states"][1], m1), distance(W["states"][2], m2)
    rules = abs(R.Du - R.S).max() / abs(R.Du).max()
    print(f"{name}: {R.nc} cells, {R.n_u} + {R.n_p} dofs; fss_tol {tol:.3e}; fixed-stress iterations {its}; d_ref step 1 u {d1[0]:.1e} p {d1[1]:.1e} eps_v {d1[2]:.1e}, "
          f"step 2 u {d2[0]:.1e} p {d2[1]:.1e} eps_v {d2[2]:.1e}; |Du - S| / |Du| = {rules:.1e}")
    assert max(its) <= 100
    assert max(d1 + d2) < 1e-9
    # the two quadrature rules of the divergence agree wherever the cells are affine (and in 2D); the non-affine 3D cells are what the model keeps both for
    assert (rules > 1e-3) if name == "jitter3_q2" else (rules <= 1e-13)


@pytest.mark.parametrize("name", list(CASES), ids=str)
def test_every_ingredient_moves_the_solution(shared, name):
    C, R, (s0, m1, m2) = shared(name)
    need = 100 * case_bound(name)
    weak = []
    for what, change in C.perturbations().items():
        Q = C.reference(**change)
        q0 = Q.initial_state()
        q1 = Q.monolithic_step(q0[0], q0[1])
        q2 = Q.monolithic_step(q1[0], q1[1])
        (u1, p1, _), (u2, p2, _) = distance(q1, m1), distance(q2, m2)
        moved = min(max(u1, p1), max(u2, p2))
        print(f"{name}: {what:45s} step 1 u {u1:.1e} p {p1:.1e}  step 2 u {u2:.1e} p {p2:.1e}   {moved / case_bound(name):8.0f} x bound")
        if moved < need:
            weak.append((what, moved))
    assert not weak, (weak, need)


@pytest.mark.parametrize("name", list(DEFAULT_REL), ids=str)
def test_default_flavour_decisions_are_clear_of_their_thresholds(shared, name):
    C, R, _ = shared(name)
    tol = DEFAULT_REL[name] * R.first_residual()
    W = R.walk(2, tol, tol, max_fss=50, max_pres=50)
    print(f"{name}: fss_tol = pressure_tol = {tol:.3e}; (fss, pressure) iterations {[(t[1], t[2]) for t in W['trace']]}; closest decision a factor {min(W['margins']):.2f} from its threshold")
    assert min(W["margins"]) >= 2.0
    assert all(t[2] < 49 for t in W["trace"]) and len(W["trace"]) < 100
    assert DT == 60.0
