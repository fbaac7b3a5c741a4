"""bench.py pieces that need no GPU: the files of --dump-outputs (float64, a fixed sample of large arrays, 64 MB at most) and the option checks."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _sizes(path):
    return sum(os.path.getsize(os.path.join(path, f)) for f in os.listdir(path))


def test_dump_outputs_whole_arrays(tmp_path):
    rng = np.random.default_rng(1)
    out = {"u": rng.standard_normal(3000), "p": rng.standard_normal(100).astype(np.float32), "trace": rng.standard_normal((2, 8))}
    bench.dump_outputs(str(tmp_path), out, 0, 1)
    assert sorted(os.listdir(tmp_path)) == ["p.npy", "trace.npy", "u.npy"]
    for k, v in out.items():
        a = np.load(tmp_path / f"{k}.npy")
        assert a.dtype == np.float64 and np.array_equal(a, v.astype(np.float64))


def test_dump_outputs_sample_large_arrays(tmp_path):
    """the largest outputs of the 72^3 bench and beyond: a fixed sample, the same from run to run, with its positions and the norms of the whole array"""
    rng = np.random.default_rng(2)
    u, p, e = rng.standard_normal(9_145_875), rng.standard_normal(3_000_000), rng.standard_normal(2_500_000)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), {"u": u, "p": p, "volumetric_strain": e, "trace": np.ones((1, 8))}, 0, 1)
        assert _sizes(tmp_path / run) <= 64 * 10 ** 6
    for name, whole in (("u", u), ("p", p), ("volumetric_strain", e)):
        idx, val = np.load(tmp_path / "a" / f"{name}_index.npy"), np.load(tmp_path / "a" / f"{name}.npy")
        assert idx.dtype == val.dtype == np.float64 and len(idx) == len(val) == 1 << 20 and np.all(np.diff(idx) > 0)
        assert np.array_equal(val, whole[idx.astype(np.int64)])
        assert np.allclose(np.load(tmp_path / "a" / f"{name}_norms.npy"), [np.linalg.norm(whole), np.abs(whole).max()])
        for f in (f"{name}.npy", f"{name}_index.npy"):
            assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


def test_dump_outputs_per_rank(tmp_path):
    rng = np.random.default_rng(3)
    for r in range(2):
        bench.dump_outputs(str(tmp_path), {"u": rng.standard_normal(3_000_000), "p": rng.standard_normal(50)}, r, 2)
    assert sorted(os.listdir(tmp_path)) == sorted(f"{n}_rank{r}.npy" for r in range(2) for n in ("u", "u_index", "u_norms", "p"))
    assert len(np.load(tmp_path / "u_rank1.npy")) == 1 << 19 and _sizes(tmp_path) <= 64 * 10 ** 6


def test_trace_out_needs_full():
    """--trace-out records the config5 block, which only --full runs: refused before anything starts"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--trace-out", os.devnull], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--full" in r.stderr, r.stderr[-1000:]
