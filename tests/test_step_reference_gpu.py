"""The time step of the device with every field on against the independent model of tests/step_reference.py: two steps of dt = 60 per case through the host driver.

Coupled / incremental flavour (pk.Runner, coupled_fss and incremental_strain set): after step 1 and after step 2 PORO_VEC_U, PORO_VEC_P and PORO_VEC_EPSV against
monolithic_step of the reference (one sparse direct solve of the backward-Euler Biot system per step), in max norm relative to the field's maximum; the prescribed
displacement and pressure dofs exactly; the hanging dofs against C applied to their masters; the six terms of Runner.flow_balance() after step 2 against
darcy_reference.balance_terms with the reference's Mp, K, src and fields.  Reference's default flavour (pk.run_problem) for three cases: trace columns 1 and 2 equal to
walk()'s, column 4 and the fields within the bound.

The device is driven with the displacement CG at 1e-14 of the norm of its first right-hand side and fss_tol = pressure_tol = 1e-10 of the first pressure residual (both
from the reference; tests/test_step_reference_cpu.py: the reference's own loop is then within 1e-9 of monolithic_step).  Bounds: 10 times the distance measured on one
MI355X, rounded up to a power of ten, none above 1e-6.  Measured (largest of u, p, eps_v over both steps; fixed-stress iterations of the two steps; CG iterations of the
displacement / pressure system summed over the run):
  run                      u, p      bound   eps_v     bound   fixed-stress   CG u / p
  box3_q2-mf               6.48e-11  1e-9    3.17e-11  1e-9    6, 6           223 / 1055
  box3_q2-csr              1.53e-10  1e-8    4.10e-09  1e-7    6, 6           224 / 1055
  box3_q2_struct-mf        6.48e-11  1e-9    3.17e-11  1e-9    6, 6           223 / 1055
  box2_q1-mf               3.01e-10  1e-8    1.34e-10  1e-8    6, 6           224 / 0 (exact line solve)
  box2_q1-csr              4.15e-10  1e-8    3.52e-09  1e-7    7, 7           244 / 64
  graded3_q2-mf            1.35e-09  1e-7    3.07e-08  1e-6    7, 7           421 / 68
  refined3_q1-mf           1.82e-09  1e-7    2.08e-07  1e-6 *  5, 5           100 / 906
  refined3_q1-mf-atomic    1.78e-09  1e-7    2.08e-07  1e-6 *  5, 5           100 / 906
  refined3_q2-mf           1.48e-09  1e-7    1.19e-07  1e-6 *  5, 5           273 / 902
  refined3_q2-mf-atomic    1.21e-09  1e-7    1.19e-07  1e-6 *  5, 5           273 / 902
  refined3_q2_hybrid-mf    6.90e-09  1e-7    3.00e-07  1e-6 *  9, 9           618 / 2802
  jitter3_q2-mf            3.41e-09  1e-7    1.99e-07  1e-6 *  6, 6           311 / 942
  jitter3_q2-csr           3.55e-09  1e-7    1.99e-07  1e-6 *  6, 6           311 / 942
  jitter2_q2-mf, -csr      2.11e-09  1e-7    3.70e-08  1e-6    9, 9           271 / 2096
  default flavour          |p|_inf   u         p         eps_v      bounds (u, p; eps_v)   (fss, pressure) iterations = walk()'s
  box3_q2-mf               3.0e-16   1.3e-14   8.1e-16   2.2e-14    1e-12; 1e-12           (1, 7), (1, 7)
  refined3_q2-mf           6.3e-15   6.5e-14   8.5e-15   3.55e-07   1e-12; 1e-6 *          (1, 5), (1, 5)
  box2_q1-csr              5.7e-16   2.1e-15   5.7e-16   3.3e-15    1e-13; 1e-13           (1, 7), (1, 7)
* eps_v is the one field that needs more than 1e-6 / 10: on these meshes the projection's mass matrix is solved by Jacobi-CG to the relative 1e-8 of the host layer's
StrainProjector control, which no run option reaches (rel_u and max_it act on the displacement solve).  The test prints the evidence: eps_v lies as far from the EXACT
projection of the device's own u (2.07e-07 on refined3_q1) as from the reference, and the summed projection residual is 2 - 4e-8 of its right-hand side; u and p, which
the loop corrects, are three orders closer.  Where the fast diagonalisation inverts the mass matrix the same field agrees to 1e-10.  These bounds stay at the 1e-6 cap,
3.3 to 8.4 times the measured value and not 10.  In the default flavour eps_v0 is projected once, at the start, and carries that error through the run.
The CPU test holds every perturbation a case switches on (relative 1e-3 of one ingredient of the reference) against 100 times these bounds."""
import numpy as np
import pytest

import poroelasticity_dealii_amd as pk
import darcy_reference as dr
import step_reference as sr
from step_reference import BOUNDS, COUPLED_REL, DEFAULT_BOUNDS, DEFAULT_REL, DT, P_INIT, Case, distance

pytestmark = pytest.mark.gpu

MF, CSR = pk.OP_MATRIX_FREE, pk.OP_CSR
# id: (case of step_reference.CASES, operator mode, run options)
RUNS = {
    "box3_q2-mf": ("box3_q2", MF, {}), "box3_q2-csr": ("box3_q2", CSR, {}),
    "box3_q2_struct-mf": ("box3_q2", MF, dict(moduli_structured=True)),
    "box2_q1-mf": ("box2_q1", MF, {}), "box2_q1-csr": ("box2_q1", CSR, {}),
    "graded3_q2-mf": ("graded3_q2", MF, {}),
    "refined3_q1-mf": ("refined3_q1", MF, {}), "refined3_q1-mf-atomic": ("refined3_q1", MF, dict(atomic_scatter=True)),
    "refined3_q2-mf": ("refined3_q2", MF, {}), "refined3_q2-mf-atomic": ("refined3_q2", MF, dict(atomic_scatter=True)),
    "refined3_q2_hybrid-mf": ("refined3_q2_hybrid", MF, dict(hybrid_operator=True)),
    "jitter3_q2-mf": ("jitter3_q2", MF, {}), "jitter3_q2-csr": ("jitter3_q2", CSR, {}),
    "jitter2_q2-mf": ("jitter2_q2", MF, {}), "jitter2_q2-csr": ("jitter2_q2", CSR, {}),
}
DEFAULT_RUNS = {"box3_q2-mf": ("box3_q2", MF), "refined3_q2-mf": ("refined3_q2", MF), "box2_q1-csr": ("box2_q1", CSR)}


class Shared:
    """per case: the problem, the reference and its two monolithic steps, computed once and left unchanged"""

    def __init__(self, tmp):
        self.tmp, self.made = tmp, {}

    def get(self, name):
        if name not in self.made:
            C = Case(name, self.tmp)
            R = C.reference()
            s0 = R.initial_state()
            m1 = R.monolithic_step(s0[0], s0[1])
            m2 = R.monolithic_step(m1[0], m1[1])
            b0 = R.CuF.T @ (R.f_ext + R.alpha * (R.Du @ s0[1]) - R.A @ R.u_fix)
            self.made[name] = dict(case=C, ref=R, steps=(s0, m1, m2), r1=R.first_residual(), b0=float(np.linalg.norm(b0)))
        return self.made[name]

    def close(self):
        for v in self.made.values():
            v["case"].close()


@pytest.fixture(scope="module")
def shared(tmp_path_factory):
    S = Shared(tmp_path_factory.mktemp("step_reference"))
    yield S
    S.close()


def controls(E, rel, max_fss):
    tol = rel * E["r1"]
    return dict(p_init=P_INIT, dt=DT, fss_tol=tol, pressure_tol=tol, max_fss=max_fss, max_pres=50, abs_u=1e-14 * E["b0"], rel_u=0.0, max_it=50000, prec=-1)


def fields(ctx):
    return ctx.get(pk.VEC_U), ctx.get(pk.VEC_P), ctx.get(pk.VEC_EPSV)


def check_constraints(R, P, u, p):
    """prescribed dofs exactly; hanging dofs = C applied to their masters (+ inhomogeneity), to rounding"""
    d = P.desc
    assert np.array_equal(u[R.dir_dof], R.dir_val)
    if len(R.pd):
        assert np.array_equal(p[R.pd], np.ctypeslib.as_array(d.dirichlet_value_p, shape=(len(R.pd),)))
    if len(R.hang_u):
        z = u.copy(); z[R.hang_u] = 0.0
        inh = sr._constraints(d.cons_u)[4]
        assert np.abs(u[R.hang_u] - ((R.Cu @ z)[R.hang_u] + inh)).max() <= 1e-14 * np.abs(u).max()
    if len(R.hang_p):
        z = p.copy(); z[R.hang_p] = 0.0
        assert np.abs(p[R.hang_p] - (R.Cp @ z)[R.hang_p]).max() <= 1e-13 * np.abs(p).max()


@pytest.mark.parametrize("run", list(RUNS), ids=str)
def test_coupled_steps_against_the_monolithic_system(shared, run):
    name, mode, options = RUNS[run]
    E = shared.get(name)
    C, R, (s0, m1, m2) = E["case"], E["ref"], E["steps"]
    kw = controls(E, COUPLED_REL, 200)
    bound, bound_ev = BOUNDS[run]
    assert bound <= 1e-6 and bound_ev <= 1e-6
    run_ = pk.Runner(C.P, operator_mode=mode, coupled_fss=True, incremental_strain=True, **kw, **options)
    try:
        run_.initialize()
        worst, worst_ev, its, cg = 0.0, 0.0, [], np.zeros(2)
        for step, ref in ((1, m1), (2, m2)):
            tr, _ = run_.step()
            assert len(tr) < 200 and tr[-1, 5] <= kw["fss_tol"], (step, len(tr), tr[-1, 5])
            u, p, ev = fields(run_.ctx)
            d = distance((u, p, ev), ref)
            its.append(len(tr)); cg += tr[:, 6:8].sum(axis=0)
            print(f"{run} step {step}: distance to monolithic_step u {d[0]:.2e} p {d[1]:.2e} eps_v {d[2]:.2e}; {len(tr)} fixed-stress iterations")
            worst, worst_ev = max(worst, d[0], d[1]), max(worst_ev, d[2])
            check_constraints(R, C.P, u, p)
            # how far eps_v is from the projection of the device's own u: what the projection's CG (relative 1e-8) leaves
            rhs = R.Cn.T @ (R.S.T @ u)
            print(f"{run} step {step}: projection residual |C^T (Mp eps_v - S^T u)| = {np.linalg.norm(R.Cn.T @ (R.Mp @ ev) - rhs) / np.linalg.norm(rhs):.2e} |C^T S^T u|, "
                  f"eps_v to the exact projection of the device's u {distance((ev,), (R.project(u),))[0]:.2e}")
        print(f"{run}: measured u, p {worst:.2e} bound {bound:g}; eps_v {worst_ev:.2e} bound {bound_ev:g}; fixed-stress iterations {its}; CG iterations u {int(cg[0])} p {int(cg[1])}")
        # the fluid balance of the state after step 2 (p_old and eps_v0: the state after step 1)
        B = run_.flow_balance()
        T = dr.balance_terms(C.P, R.Mp, R.Kp, R.src, m2[1], m1[1], m2[2], m1[2], DT)
        for key in ("storage_rate_strain", "storage_rate_pressure", "source_sum", "outflow_prescribed"):
            e = abs(B[key] - T["terms"][key]) / T["scales"][key]
            print(f"{run} {key}: device {B[key]:.6e} reference {T['terms'][key]:.6e} difference {e:.2e} of the sum of absolute values")
            assert e <= (bound_ev if key == "storage_rate_strain" else bound), (key, B[key], T["terms"][key])
        # the two terms that vanish with the loop's residual: the loop's own criterion and Cauchy-Schwarz (include/poroel_hip.h); the identity closes to rounding
        assert B["residual_l2"] <= kw["fss_tol"] and abs(B["free_row_sum"]) <= np.sqrt(R.n_p) * B["residual_l2"] * (1 + 1e-12)
        closed = B["storage_rate_strain"] + B["storage_rate_pressure"] + B["source_sum"] + B["outflow_prescribed"] + B["free_row_sum"]
        assert abs(closed) <= 1e-12 * T["scale"], (closed, T["scale"])
        assert worst <= bound and worst_ev <= bound_ev, (worst, bound, worst_ev, bound_ev)
    finally:
        run_.close()


@pytest.mark.parametrize("run", list(DEFAULT_RUNS), ids=str)
def test_default_flavour_against_the_walked_loop(shared, run):
    name, mode = DEFAULT_RUNS[run]
    E = shared.get(name)
    C, R = E["case"], E["ref"]
    kw = controls(E, DEFAULT_REL[name], 50)
    bound, bound_ev = DEFAULT_BOUNDS[run]
    assert bound <= 1e-6 and bound_ev <= 1e-6
    W = R.walk(2, kw["fss_tol"], kw["pressure_tol"], max_fss=50, max_pres=50)
    tr, G = pk.run_problem(C.P, 2, kw.pop("p_init"), kw.pop("dt"), operator_mode=mode, **kw)
    try:
        rows = tr[1:]
        print(f"{run}: device rows {[(int(r[1]), int(r[2])) for r in rows]} reference rows {[(t[1], t[2]) for t in W['trace']]}")
        assert [(int(r[0]), int(r[1]), int(r[2])) for r in rows] == [t[:3] for t in W["trace"]]
        e_inf = max(abs(r[4] - t[3]) / t[3] for r, t in zip(rows, W["trace"]))
        d = distance(fields(G), W["states"][-1])
        print(f"{run}: measured |p|_inf {e_inf:.2e}, distance to walk() u {d[0]:.2e} p {d[1]:.2e} bound {bound:g}; eps_v {d[2]:.2e} bound {bound_ev:g}")
        assert e_inf <= bound and max(d[0], d[1]) <= bound and d[2] <= bound_ev
        check_constraints(R, C.P, G.get(pk.VEC_U), G.get(pk.VEC_P))
    finally:
        G.close()
