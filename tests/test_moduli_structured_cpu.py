"""Structured box operator for layered per-cell moduli, without a GPU: the per-plane weight table (csrc/moduli_planes.hpp, through a small stand-alone program built
with the address and undefined-behaviour sanitizers), the weighted 1D bands rebuilt from it the way the kernel's z-stage combines them, and the Kronecker form of the
operator against the per-cell quadrature assembly of the reference.

Bounds: 1e-14 relative for the 1D bands (a handful of exactly representable integer coefficients times a weight: one or two roundings per entry); 1e-13 of max|A| for
the Kronecker identity (an entry of the reference is a sum over up to 8 cells x 27 quadrature points, about 2e-14 of accumulated rounding in the worst case)."""
import subprocess

import numpy as np
import pytest

import poroelasticity_dealii_amd as pk
from common import BC_3D, build_sanitized_check, material
from moduli_reference import ModuliReference, fe1d_weighted, layer_decades, per_cell

# integer element matrices and their scales (the header of csrc/kernels_kron.hip): M = sM Mi, K = sK Ki, C = sC Ci with C[m][n] = int phi_m' phi_n
ELEMENT = {
    2: (np.array([[4, 2, -1], [2, 16, 2], [-1, 2, 4]], float), np.array([[7, -8, 1], [-8, 16, -8], [1, -8, 7]], float), np.array([[-3, -4, 1], [4, 0, -4], [-1, 4, 3]], float),
        lambda h: h / 30.0, lambda h: 1.0 / (3.0 * h), 1.0 / 6.0),
    1: (np.array([[2, 1], [1, 2]], float), np.array([[1, -1], [-1, 1]], float), np.array([[-1, -1], [1, 1]], float), lambda h: h / 6.0, lambda h: 1.0 / h, 0.5),
}


def c1d_weighted(k, n, w):
    """dense C^w = sum_l w_l C_l of a line of n cells (independent of the cell size)"""
    Ci, sC = ELEMENT[k][2], ELEMENT[k][5]
    C = np.zeros((k * n + 1, k * n + 1))
    for e in range(n):
        s = slice(k * e, k * e + k + 1)
        C[s, s] += w[e] * sC * Ci
    return C


def plane_table(exe, k, lam, G):
    out = subprocess.run([exe, str(k)] + [repr(float(v)) for v in np.r_[lam, G]], check=True, capture_output=True, text=True).stdout.split()
    return np.array([float(v) for v in out]).reshape(k * len(lam) + 1, 4)


def bands_from_table(k, table, pick):
    """dense integer-scaled (M^w, K^w, C^w) of the line, row by row the way the kernel's z-stage forms them: a vertex plane adds the one-sided halves of its row (the
    last row of the element below, the first row of the element above), each times that side's weight; a mid plane (Q2) takes its layer's weight.
    pick(lambda, G) -> the weight"""
    Mi, Ki, Ci = ELEMENT[k][:3]
    n = len(table)
    out = [np.zeros((n, n)) for _ in range(3)]
    for p in range(n):
        wlo, whi = pick(table[p, 0], table[p, 1]), pick(table[p, 2], table[p, 3])
        for A, E in zip(out, (Mi, Ki, Ci)):
            if p % k:                                                      # mid plane: the element's middle row, nodes p - 1 .. p + 1
                assert wlo == whi
                A[p, p - 1:p + 2] += wlo * E[1]
            else:
                if p > 0:
                    A[p, p - k:p + 1] += wlo * E[k]
                else:
                    assert wlo == 0.0                                      # no layer below the box
                if p < n - 1:
                    A[p, p:p + k + 1] += whi * E[0]
                else:
                    assert whi == 0.0
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_sanitized_check(tmp_path_factory.mktemp("moduli_planes"), "moduli_planes_check")


@pytest.mark.parametrize("n_layers", [1, 2, 5])
@pytest.mark.parametrize("k", [1, 2])
def test_plane_table_rebuilds_the_weighted_bands(exe, k, n_layers):
    lam, G = layer_decades(material(), n_layers)
    table = plane_table(exe, k, lam, G)
    h = 0.7
    _, _, _, sM, sK, sC = ELEMENT[k]
    for name, pick, w in (("lambda", lambda a, b: a, lam), ("G", lambda a, b: b, G), ("lambda+2G", lambda a, b: a + 2 * b, lam + 2 * G)):
        Mw, Kw, Cw = bands_from_table(k, table, pick)
        M0, K0 = fe1d_weighted(k, np.full(n_layers, h), w)
        C0 = c1d_weighted(k, n_layers, w)
        for got, want, what in ((sM(h) * Mw, M0, "M"), (sK(h) * Kw, K0, "K"), (sC * Cw, C0, "C")):
            e = np.abs(got - want).max() / np.abs(want).max()
            assert e <= 1e-14, (k, n_layers, name, what, e)
        # the diagonal of C^w at an interface is (w_below - w_above) / 2 for either degree (3 (w_lo - w_hi) / 6 for Q2): non-zero wherever the weight jumps
        for l in range(1, n_layers):
            assert sC * Cw[k * l, k * l] == pytest.approx((w[l - 1] - w[l]) / 2, rel=1e-14)


def kronecker_operator(k, n, size, lam, G):
    """A_u of a uniform box with lambda, G per cell layer of z, node-interleaved lexicographic dofs, from 1D matrices alone:
    A_aa = sum_d F_x (x) F_y (x) F_z^w, w = lambda + 2G (d == a) | G, F_d = K, the others M;  A_ab = C_a (x) C_b^T [lambda] + C_a^T (x) C_b [G], M in the third direction"""
    one = [np.ones(n[d]) for d in range(3)]
    h = [np.full(n[d], size[d] / n[d]) for d in range(3)]
    nn = [k * n[d] + 1 for d in range(3)]

    def mats(d, w):
        M, K = fe1d_weighted(k, h[d], w)
        return {"M": M, "K": K, "C": c1d_weighted(k, n[d], w), "T": c1d_weighted(k, n[d], w).T}

    def kron3(fx, fy, fz, w):                                              # the weight sits on the z factor
        return np.kron(mats(2, w)[fz], np.kron(mats(1, one[1])[fy], mats(0, one[0])[fx]))
    N = nn[0] * nn[1] * nn[2]
    A = np.zeros((3 * N, 3 * N))
    for a in range(3):
        for d in range(3):
            f = ["M", "M", "M"]; f[d] = "K"
            A[a::3, a::3] += kron3(*f, lam + 2 * G if d == a else G)
        for b in range(3):
            if a == b:
                continue
            f = ["M", "M", "M"]; f[a] = "C"; f[b] = "T"
            g = ["M", "M", "M"]; g[a] = "T"; g[b] = "C"
            A[a::3, b::3] += kron3(*f, lam) + kron3(*g, G)
    return A


@pytest.mark.parametrize("k,n", [(2, [2, 1, 3]), (1, [3, 2, 4])], ids=["q2-2x1x3", "q1-3x2x4"])
def test_kronecker_form_is_the_per_cell_assembly(k, n):
    m = material()
    size = [2.0, 1.5, 2.4]
    P = pk.Problem.box(3, n, size, k, m, BC_3D)
    try:
        rng = np.random.default_rng(11)
        lam, G = m.lame_lambda * 10.0 ** rng.uniform(-3, 0, n[2]), m.shear_G * 10.0 ** rng.uniform(-3, 0, n[2])      # random over three decades per layer
        A0 = ModuliReference(P, per_cell(P, lam), per_cell(P, G)).assemble_full().toarray()
        A = kronecker_operator(k, n, size, lam, G)
        e = np.abs(A - A0).max() / np.abs(A0).max()
        print(f"Q{k} {n}: Kronecker form vs per-cell quadrature assembly {e:.2e} of max|A|")
        assert e <= 1e-13
    finally:
        P.close()


def test_symbols_and_constants():
    hip = pk.load_hip()
    for s in ("poro_ctx_set_moduli_operator", "poro_ctx_get_moduli_operator"):
        assert s in pk.HIP_SYMBOLS and getattr(hip, s)
    assert (pk.MODULI_OP_CELLS, pk.MODULI_OP_STRUCTURED) == (0, 1) and hip.poro_abi_version() == 4
