"""CPU companion of the slab-partition tests (tests/test_slab_fdm_gpu.py, tests/test_slab_iterates_gpu.py; no GPU): the helper's window / stitch bookkeeping on uneven
slabs, its restatement of the slab form's chunk and share arithmetic against values computed by hand, and the soundness of the reference alone on the new shapes - thin,
long boxes and the mixed Dirichlet list - where BoxReference.block_inverse_u must equal component-wise sparse direct solves of the oracle's assembled matrix (the bound of
tests/test_box_reference_cpu.py for the same comparison, 1e-11)."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

import poroelasticity_dealii_amd as pk
import oracle_py
import slab_ranks as sr
from box_reference import BoxReference
from common import csr_to_scipy


@pytest.mark.parametrize("dim,n,deg,world", [(3, (4, 3, 7), 2, 3), (3, (3, 2, 24), 2, 5), (3, (3, 2, 40), 2, 8), (2, (2, 9), 1, 4), (2, (6, 9), 2, 3), (3, (5, 4, 9), 1, 3)], ids=str)
def test_windows_and_stitch_round_trip_on_uneven_slabs(dim, n, deg, world):
    S = sr.Slabs(dim, n, deg, world)
    G = sr.Slabs(dim, n, deg, 1)
    try:
        assert sum(S.layers) == n[-1] and min(S.layers) >= 1 and (n[-1] % world == 0 or len(set(S.layers)) > 1)
        assert (S.N_u, S.N_p) == (G.n_u[0], G.n_p[0])
        nn = [deg * m + 1 for m in n]
        assert S.plane_u == dim * int(np.prod(nn[:-1])) and S.plane_p == int(np.prod([m + 1 for m in n[:-1]]))
        # a window starts at the first node plane of the rank's first cell layer
        first = np.concatenate([[0], np.cumsum(S.layers)[:-1]])
        assert S.off_u == [int(deg * f * S.plane_u) for f in first] and S.off_p == [int(f * S.plane_p) for f in first]
        for N, win, stitch, plane in ((S.N_u, S.window_u, S.stitch_u, S.plane_u), (S.N_p, S.window_p, S.stitch_p, S.plane_p)):
            x = np.random.default_rng(5).standard_normal(N)
            parts = [win(x, r) for r in range(world)]
            assert np.array_equal(stitch(parts), x)
            for a, b in sr.shared_copies(parts, plane):
                assert a.size == plane and np.array_equal(a, b)
            parts[1] = parts[1].copy(); parts[1][0] += 1.0             # rank 1's copy of the first interface: stitch takes rank 0's, shared_copies sees the difference
            a, b = sr.shared_copies(parts, plane)[0]
            assert not np.array_equal(a, b) and np.array_equal(stitch(parts), x)
        # the coordinates of a rank's vertices are the window of the global ones: the numbering is the one the offsets assume
        Xg = G.problems[0].array("vertex_coords", (G.problems[0].desc.n_vertices, dim))
        for r, P in enumerate(S.problems):
            X = P.array("vertex_coords", (P.desc.n_vertices, dim))
            assert np.allclose(X, Xg[S.off_p[r]: S.off_p[r] + S.n_p[r]], rtol=0, atol=1e-12)
    finally:
        S.close(); G.close()


def test_a_dead_rank_aborts_the_others():
    def fn(r, comm):
        if r == 1:
            raise ValueError("rank 1 dies")
        comm.barrier.wait()
    with pytest.raises(RuntimeError, match="rank 1 dies"):
        sr.run_collectively(3, fn)


def test_chunk_and_share_arithmetic_by_hand():
    """(3,2,24) Q2 on 5 ranks: 7 x 5 x 49 nodes; half lines 4, 3 and 25 -> 2 tiles, both-parity z pass, chunks of 16 columns; a plane of 4 x 3 = 12 positions is one chunk, 12
    blocks -> 12 chunks, 3 per rank: ranks 0 .. 3 hold 3 each and the last rank's share is empty"""
    L = sr.slab_shares((3, 2, 24), 2, 5)
    assert L == dict(nt=2, zboth=True, cw=16, nchunk=1, chunk_total=12, cps=3, my_chunks=[3, 3, 3, 3, 0], scols=48, col_unit=16, share_at_least_a_block=True, straddling=[])
    # (3,2,40) on 8 ranks: half line 41 -> 3 tiles, chunks of 48 columns, 12 chunks, 2 per rank: the last two shares are empty
    L = sr.slab_shares((3, 2, 40), 2, 8)
    assert (L["nt"], L["zboth"], L["cw"], L["cps"], L["my_chunks"]) == (3, False, 48, 2, [2, 2, 2, 2, 2, 2, 0, 0])
    # (3,3,16) on 5 ranks, the box of the iterate tests: 7 x 7 x 33 nodes, half lines 4, 4, 17 -> the same 2 tiles, one chunk per block, 3 per rank and an empty last share
    L = sr.slab_shares((3, 3, 16), 2, 5)
    assert (L["nt"], L["zboth"], L["nchunk"], L["cps"], L["my_chunks"]) == (2, True, 1, 3, [3, 3, 3, 3, 0])
    # the two-workgroup switch widens the chunk to a whole block of 32 columns
    L = sr.slab_shares((3, 2, 24), 2, 2, two_parity_workgroups=True)
    assert (L["zboth"], L["cw"], L["cps"], L["scols"]) == (False, 32, 6, 192)
    # (6,5,7) on 5 ranks: 13 x 11 x 15 nodes, half lines 7 (pitch 8), 6, 8 -> 1 tile; plane 48 = 3 chunks of 16; 36 chunks, 8 per rank (the last: 4); share 128 columns,
    # block 48: block 2 = columns 96 .. 143 lies in shares 0 and 1, block 5 = 240 .. 287 in shares 1 and 2, block 7 = 336 .. 383 stays in share 2, block 8 = 384 .. 431 starts share 3
    L = sr.slab_shares((6, 5, 7), 2, 5)
    assert (L["nt"], L["nchunk"], L["cps"], L["my_chunks"], L["scols"], L["col_unit"], L["straddling"]) == (1, 3, 8, [8, 8, 8, 8, 4], 128, 48, [2, 5, 10])
    # the fused Q1 form of (10,9,8) on 3 ranks: 11 x 10 x 9 vertices -> 1 tile, plane 110 = 7 chunks of 16, 3 per rank (the last: 1): a share (48) is shorter than the block (112)
    L = sr.slab_shares((10, 9, 8), 1, 3, scalar=True)
    assert (L["nt"], L["nchunk"], L["cps"], L["my_chunks"], L["scols"], L["col_unit"], L["share_at_least_a_block"]) == (1, 7, 3, [3, 3, 1], 48, 112, False)
    assert sr.max_tiles() == 8
    # the nodal distributed form: columns in groups of ceil(ncol / W); 2D (2,9) Q1 on 4 ranks has 3 columns, one each, none for the last rank
    assert sr.nodal_columns((2, 9), 1, 2, 4) == [1, 1, 1, 0]
    assert sr.nodal_columns((6, 9), 2, 2, 3) == [5, 5, 3]


def test_the_shapes_visit_the_layout_edges_they_are_named_for():
    for name, (dim, n, deg, world, bc, env, form, nt) in sr.FDM_U_CASES.items():
        if form != "slab":
            continue
        L = sr.slab_shares(n, deg, world, two_parity_workgroups=bool(env))
        assert L["nt"] == nt, (name, L)
        assert L["zboth"] == (nt in (2, 4, 5) and not env), (name, L)
        assert ("empty_share" in name) == (min(L["my_chunks"]) == 0), (name, L)
        assert L["share_at_least_a_block"], name      # 12 blocks: cps = ceil(12 nchunk / W) >= nchunk up to 12 ranks - the per-column division is reached by the fused Q1 form only
    assert {sr.FDM_U_CASES[k][7] for k in sr.FDM_U_CASES if sr.FDM_U_CASES[k][6] == "slab"} == set(range(1, sr.max_tiles() + 1))
    # planes larger than a chunk: shares that end on block boundaries, and one whose blocks lie in two shares
    lay = {k: sr.slab_shares(*sr.FDM_U_CASES[k][1:4]) for k in sr.PLANE_CASES}
    assert all(L["nchunk"] > 1 for L in lay.values())
    assert any(L["straddling"] for L in lay.values()) and any(not L["straddling"] for L in lay.values())
    # the long box is beyond the kernels' reach: its half line needs more tiles than the pass kernel has
    assert sr.slab_shares((2, 2, 130), 2, 2)["nt"] > sr.max_tiles()


SHAPES = sorted({(dim, n, deg, None if bc is None else tuple(bc)) for dim, n, deg, world, bc, env, form, nt in sr.FDM_U_CASES.values()}, key=str)


@pytest.mark.parametrize("dim,n,deg,bc", SHAPES, ids=lambda v: "mixed" if isinstance(v, tuple) and v and isinstance(v[0], tuple) else str(v))
def test_block_inverse_of_the_reference_on_the_new_shapes(dim, n, deg, bc):
    P = sr.problem(dim, n, deg, bc=None if bc is None else list(bc))
    O = oracle_py.Oracle(P, hoisted=True)
    try:
        R = BoxReference(P)
        O.fill(pk.VEC_P, 0.0); O.disp_assemble_system(True)
        A = csr_to_scipy(*O.export_csr(pk.MAT_A_U))
        g = np.random.default_rng(11).standard_normal(R.n_u) * 1e3; g[R.mask] = 0.0
        z0 = np.zeros_like(g)
        for c in range(dim):
            idx = np.arange(c, R.n_u, dim); idx = idx[~R.mask[idx]]
            z0[idx] = spla.splu(A[idx][:, idx].tocsc()).solve(g[idx])
        e = np.abs(R.block_inverse_u(g) - z0).max() / np.abs(z0).max()
        print(f"{dim}d {n} Q{deg}: block_inverse_u against sparse direct solves {e:.2e}")
        assert e <= 1e-11
        assert np.abs(R.diag_A() - A.diagonal()).max() <= 1e-13 * np.abs(A.diagonal()).max()
    finally:
        O.close(); P.close()
