"""The gfx950 code of the octant-form transform pass (no GPU needed: hipcc cross-compiles): every fp32 instantiation (k_fdmo_pass_f32) runs on the f32 16x16x4
MFMA and holds no fp64 MFMA, every fp64 instantiation (k_fdmo_pass) holds no f32 MFMA, and none of them uses scratch memory."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "poroelasticity_dealii_amd", "csrc", "kernels_fdmo.hip")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return r.stdout.split("\n")[:len(names)]


@pytest.mark.skipif(HIPCC is None or shutil.which("c++filt") is None, reason="hipcc / c++filt not installed")
def test_pass_instantiations_use_the_mfma_of_their_precision_and_no_scratch(tmp_path):
    out = str(tmp_path / "kernels_fdmo.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", SRC, "-o", out], check=True, timeout=900)
    text = open(out).read()
    mangled = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)
    kernels = dict(zip(mangled, demangle(mangled)))
    seen = {"fp32": 0, "fp64": 0}
    for sym, name in kernels.items():
        m = re.search(r"\b(k_fdmo_pass(?:_f32)?)<", name)
        if not m:
            continue
        body = re.search(r"^" + re.escape(sym) + r":.*?\n(.*?)^\.Lfunc_end\d+:", text, flags=re.M | re.S)
        desc = re.search(r"^\s*\.amdhsa_kernel\s+" + re.escape(sym) + r"\n(.*?)^\s*\.end_amdhsa_kernel", text, flags=re.M | re.S)
        assert body and desc, name
        code = body.group(1)
        f32 = re.findall(r"^\s*(v_mfma_f32_16x16x4_?f32)\b", code, flags=re.M)
        f64 = re.findall(r"^\s*(v_mfma_f64\w*)", code, flags=re.M)
        scratch = re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", desc.group(1))
        assert scratch and int(scratch.group(1)) == 0, (name, scratch and scratch.group(1))
        if m.group(1) == "k_fdmo_pass_f32":
            assert f32 and not f64, (name, len(f32), len(f64))
            seen["fp32"] += 1
        else:
            assert f64 and not f32, (name, len(f32), len(f64))
            seen["fp64"] += 1
    # 8 tile counts x (pass 1, pass 2, pass 2 with g . z, pass 3) in fp32; the fp64 kernel has those and its slab / general variants
    assert seen["fp32"] == 32 and seen["fp64"] >= 32, seen
