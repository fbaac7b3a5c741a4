"""Scaffolding of the slab-partition tests: W ranks of a slab-partitioned box as W threads of one process (tools/rank_threads.py: ThreadComm, box_problem), a per-rank
callable run collectively on them, and the bookkeeping between the global vectors of the single-rank box and the ranks' windows.

A slab holds whole node planes of the last direction; the upper plane of rank r is the lower plane of rank r + 1 (`plane_u` / `plane_p` dofs, poro_partition).  So the
window of rank r starts at sum_{q < r} (n_q - plane) of the global numbering, as tests/mr_worker.py computes it, and the global vector is the ranks' windows with every
shared plane taken once (`stitch`).

`slab_shares` restates, on the host, the chunk and share arithmetic of the slab form of the transform kernels (kernels_fdmo.hip: form_geometry, slab_layout and the
destination computation of the passes), from the cell counts alone: the tests use it to assert which layout edge a shape visits."""
import os
import re
import sys
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (os.path.join(ROOT, "tools"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import poroelasticity_dealii_amd as pk  # noqa: E402
import rank_threads                     # noqa: E402
from rank_threads import ThreadComm     # noqa: E402

CSRC = os.path.join(ROOT, "poroelasticity_dealii_amd", "csrc")


def max_tiles():
    """kFdmoMaxTiles of fdm_tables.hpp: 16-wide tiles per transformed line the pass kernel is instantiated for"""
    with open(os.path.join(CSRC, "fdm_tables.hpp")) as f:
        found = re.findall(r"constexpr\s+int\s+kFdmoMaxTiles\s*=\s*(\d+)\s*;", f.read())
    assert len(found) == 1, found
    return int(found[0])


def problem(dim, n, deg, rank=0, n_ranks=1, bc=None):
    """rank_threads.box_problem, or the same box with another Dirichlet list"""
    if bc is None:
        return rank_threads.box_problem(dim, n, deg, rank=rank, n_ranks=n_ranks)
    return pk.Problem.box(dim, list(n), [10.0] * dim, deg, rank_threads.bench.material(), list(bc), (), rank, n_ranks)


def offsets(sizes, plane):
    """global index of the first entry of every rank's window: the windows overlap by one plane"""
    off = [0]
    for m in sizes[:-1]:
        off.append(off[-1] + m - plane)
    return off


def window(x, off, size):
    return np.ascontiguousarray(x[off: off + size])


def stitch(parts, plane):
    """global vector from the ranks' windows: the upper shared plane of rank r is the lower one of rank r + 1 and is taken from rank r (`shared_copies` compares the two)"""
    return rank_threads.stitch(list(parts), plane)


def shared_copies(parts, plane):
    """[(upper plane of rank r, lower plane of rank r + 1)] for every interface"""
    return [(a[len(a) - plane:], b[:plane]) for a, b in zip(parts[:-1], parts[1:])]


class Slabs:
    """the W slabs of one box: the ranks' problems, window offsets of both spaces, and the collective runner"""

    def __init__(self, dim, n, deg, world, bc=None):
        self.dim, self.n, self.deg, self.world, self.bc = dim, tuple(n), deg, world, bc
        self.problems = [problem(dim, n, deg, r, world, bc) for r in range(world)]
        d = [P.desc for P in self.problems]
        self.plane_u, self.plane_p = int(d[0].part.plane_u), int(d[0].part.plane_p)
        self.n_u, self.n_p = [int(x.n_dofs_u) for x in d], [int(x.n_dofs_p) for x in d]
        self.layers = [int(x.box.n[dim - 1]) for x in d]
        self.off_u, self.off_p = offsets(self.n_u, self.plane_u), offsets(self.n_p, self.plane_p)
        self.N_u, self.N_p = self.off_u[-1] + self.n_u[-1], self.off_p[-1] + self.n_p[-1]

    def close(self):
        for P in self.problems:
            P.close()
        self.problems = []

    def window_u(self, x, r):
        return window(x, self.off_u[r], self.n_u[r])

    def window_p(self, x, r):
        return window(x, self.off_p[r], self.n_p[r])

    def stitch_u(self, parts):
        out = stitch(parts, self.plane_u)
        assert out.size == self.N_u
        return out

    def stitch_p(self, parts):
        out = stitch(parts, self.plane_p)
        assert out.size == self.N_p
        return out

    def run(self, fn):
        """fn(rank, problem, comm) on every rank thread, collectively; returns the ranks' results.  A rank that raises aborts the barrier, so the others do not wait
        for ever, and the first failure is raised here"""
        return run_collectively(self.world, lambda r, comm: fn(r, self.problems[r], comm))


def run_collectively(world, fn):
    comm = ThreadComm(world)
    out, errs = [None] * world, []

    def rank_main(r):
        try:
            out[r] = fn(r, comm)
        except BaseException as exc:   # noqa: BLE001 - a dead rank must not leave the others waiting for ever
            errs.append((r, exc))
            comm.barrier.abort()
            for (a, b), q in comm.mail.items():      # ... nor in a pairwise exchange with it
                if a == r:
                    q.put(np.zeros(0))

    th = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    if errs:
        first = [e for e in errs if not isinstance(e[1], threading.BrokenBarrierError)] or errs
        raise RuntimeError(f"rank threads failed: {[(r, repr(e)) for r, e in errs]}") from first[0][1]
    return out


def context(P, r, comm, mode=pk.OP_MATRIX_FREE):
    """the rank's context with the thread communicator's callbacks"""
    G = pk.Context(P, 0, mode)
    if comm.n > 1:
        G.comm_callbacks(lambda b: comm.allreduce(r, b), lambda s, v, peer: comm.sendrecv(r, s, v, peer))
    return G


# ---- the layout of the slab form, restated ----------------------------------------------------------------------------------------------------------------------------
def slab_shares(n, deg, world, scalar=False, two_parity_workgroups=False):
    """kernels_fdmo.hip for a 3D box of n cells on `world` slabs: form_geometry (tile count), slab_layout (chunks, shares) and the destination computation of passes 1 / 3.
    scalar: the fused Q1 form (whole lines, one block) instead of the quadrant form of the displacement system (x, y and the global z line split in parities, 12 blocks =
    3 components x 4 quadrants).  A chunk is `cw` plane positions of one block; rank q transforms chunks [q cps, (q + 1) cps) = its share of `scols` columns; a block's
    plane positions are `col_unit` consecutive columns.  The passes take one of two destination computations: scols >= col_unit (a block lies in at most two shares: two
    bases) or the division per column.  straddling: the blocks whose columns lie in two shares (first computation only: the second base is used)"""
    nn = [deg * m + 1 for m in n]
    assert len(nn) == 3
    ng = nn[2]
    if scalar:
        h, hxp, hmax, nb, parts = nn[:2], nn[0], max(nn), 1, 1
    else:
        h = [(nn[0] + 1) // 2, (nn[1] + 1) // 2]
        hxp, hmax, nb, parts = (h[0] + 1) & ~1, max((ng + 1) // 2, h[0], h[1]), 12, 2
    nt = (hmax + 15) // 16
    zboth = parts == 2 and nt in (2, 4, 5) and not two_parity_workgroups
    chunk = 64 if nt == 5 else 16 * nt
    cw = chunk // 2 if zboth else chunk
    pl = hxp * h[1]
    nchunk = (pl + cw - 1) // cw
    chunk_total = nb * nchunk
    cps = (chunk_total + world - 1) // world
    my_chunks = [max(0, min(cps, chunk_total - r * cps)) for r in range(world)]
    scols, col_unit = cps * cw, nchunk * cw
    straddling = [co for co in range(nb) if scols >= col_unit and (co * col_unit) // scols != ((co + 1) * col_unit - 1) // scols]
    return dict(nt=nt, zboth=zboth, cw=cw, nchunk=nchunk, chunk_total=chunk_total, cps=cps, my_chunks=my_chunks, scols=scols, col_unit=col_unit,
                share_at_least_a_block=scols >= col_unit, straddling=straddling)


def nodal_columns(n, deg, dim, world, q1=False):
    """ctx_prec.hip, the nodal distributed form: the columns (nodes of one plane) are dealt out in groups of C = ceil(ncol / W); ncols_of(q) per rank"""
    k = 1 if q1 else deg
    ncol = int(np.prod([k * m + 1 for m in n[:dim - 1]]))
    C = (ncol + world - 1) // world
    return [max(0, min(C, ncol - q * C)) for q in range(world)]


# ---- the shapes of tests/test_slab_fdm_gpu.py, shared with the CPU companion (tests/test_slab_reference_cpu.py) ------------------------------------------------------------
MIXED_3D = [(0, 0, 0.0), (1, 0, -1e-5), (2, 1, 0.0), (3, 1, -1e-5), (4, 2, 0.0), (2, 0, 2e-6), (5, 1, 0.0)]     # as tests/test_fdm_u_gpu.py: different end conditions along a line
TWO_WG = {"PORO_FDMO_SLAB_TWO_PARITY_WORKGROUPS": "1"}
# name -> (dim, cells, degree, ranks, Dirichlet list or None = the benchmark's, environment, form: "slab" | "nodal", tiles per half line or None)
FDM_U_CASES = {
    "nt1_4x3x7_w3": (3, (4, 3, 7), 2, 3, None, {}, "slab", 1),
    "nt2_3x2x24_w2": (3, (3, 2, 24), 2, 2, None, {}, "slab", 2),
    "nt2_3x2x24_w5_empty_share": (3, (3, 2, 24), 2, 5, None, {}, "slab", 2),
    "nt3_3x2x40_w3": (3, (3, 2, 40), 2, 3, None, {}, "slab", 3),
    "nt3_3x2x40_w8_empty_shares": (3, (3, 2, 40), 2, 8, None, {}, "slab", 3),
    "nt4_2x3x48_w4": (3, (2, 3, 48), 2, 4, None, {}, "slab", 4),
    "nt5_3x2x72_w3": (3, (3, 2, 72), 2, 3, None, {}, "slab", 5),
    "nt6_2x2x88_w2": (3, (2, 2, 88), 2, 2, None, {}, "slab", 6),
    "nt7_2x2x104_w3": (3, (2, 2, 104), 2, 3, None, {}, "slab", 7),
    "nt8_2x2x120_w2": (3, (2, 2, 120), 2, 2, None, {}, "slab", 8),
    "nt2_3x2x24_w2_two_wg": (3, (3, 2, 24), 2, 2, None, TWO_WG, "slab", 2),
    "nt4_2x3x48_w4_two_wg": (3, (2, 3, 48), 2, 4, None, TWO_WG, "slab", 4),
    "nt5_3x2x72_w3_two_wg": (3, (3, 2, 72), 2, 3, None, TWO_WG, "slab", 5),
    "plane_10x9x24_w3": (3, (10, 9, 24), 2, 3, None, {}, "slab", 2),
    "plane_9x10x12_w4": (3, (9, 10, 12), 2, 4, None, {}, "slab", 1),
    "plane_6x5x7_w5_straddling": (3, (6, 5, 7), 2, 5, None, {}, "slab", 1),
    "q1_5x4x9_w3": (3, (5, 4, 9), 1, 3, None, {}, "slab", 1),
    "nodal_no_oct_4x3x7_w3": (3, (4, 3, 7), 2, 3, None, {"PORO_FDMU_NO_OCT": "1"}, "nodal", None),
    "nodal_mixed_3x4x6_w3": (3, (3, 4, 6), 2, 3, MIXED_3D, {}, "nodal", None),
    "nodal_long_2x2x130_w2": (3, (2, 2, 130), 2, 2, None, {}, "nodal", None),
    "nodal_2d_6x9_w3": (2, (6, 9), 2, 3, None, {}, "nodal", None),
    "nodal_2d_q1_2x9_w4": (2, (2, 9), 1, 4, None, {}, "nodal", None),
}
PLANE_CASES = ("plane_10x9x24_w3", "plane_9x10x12_w4", "plane_6x5x7_w5_straddling")
