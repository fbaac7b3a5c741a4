"""The gfx950 code of the general cell-loop kernels (no GPU needed: hipcc cross-compiles): every atomic-scatter instantiation adds with the hardware
instruction global_atomic_add_f64 and holds no compare-and-swap loop; no coloured instantiation holds an atomic of any kind."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "poroelasticity_dealii_amd", "csrc", "kernels_mfg.hip")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return r.stdout.split("\n")[:len(names)]


def is_atomic(name):
    """k_mfg<DIM, true>, k_mfg3_sf<N1, AFFINE, 1 | 2>, k_mfg2_sf<N1, 1> (2: the transposed form of the 3D kernels, PORO_MFG_ATOMIC_SHAPE)"""
    m = re.search(r"(k_mfg\w*)<([^>]*)>", name)
    assert m, name
    last = m.group(2).split(",")[-1].strip()
    return last == "true" if m.group(1) == "k_mfg" else last in ("1", "2")


@pytest.mark.skipif(HIPCC is None or shutil.which("c++filt") is None, reason="hipcc / c++filt not installed")
def test_atomic_instantiations_use_the_hardware_add(tmp_path):
    out = str(tmp_path / "kernels_mfg.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", SRC, "-o", out], check=True, timeout=900)
    text = open(out).read()
    mangled = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)
    kernels = dict(zip(mangled, demangle(mangled)))
    assert len(kernels) == 20, sorted(kernels.values())          # 8 coloured (as before the mode existed) + their 8 atomic twins + the 4 transposed 3D forms
    seen = {True: 0, False: 0}
    for sym, name in kernels.items():
        body = re.search(r"^" + re.escape(sym) + r":.*?\n(.*?)^\.Lfunc_end\d+:", text, flags=re.M | re.S)
        assert body, name
        code = body.group(1)
        atomics = re.findall(r"^\s*((?:global|flat|buffer|ds)_\w*atomic\w*|\w*cmpswap\w*)", code, flags=re.M)
        if is_atomic(name):
            assert "global_atomic_add_f64" in code, name
            assert not any("cmpswap" in a for a in atomics), (name, atomics)
            assert set(atomics) == {"global_atomic_add_f64"}, (name, set(atomics))
        else:
            assert not atomics, (name, atomics)
        seen[is_atomic(name)] += 1
    assert seen == {True: 12, False: 8}, seen
