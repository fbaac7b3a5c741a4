#!/usr/bin/env python3
"""Compare the kernels of two AMDGPU assembly files (hipcc --cuda-device-only -S): symbol sets, then per kernel either the whole
text (function body + .amdhsa_kernel descriptor; default) or, with --resources, the figures that decide occupancy.
Only the function-index part of local labels (.LBB<n>_, .Lfunc_end<n>, and the "Header=BB<n>_" of loop comments) is normalised; instantiation order does not matter."""
import re
import sys

FIGURES = ("next_free_vgpr", "accum_offset", "private_segment_fixed_size", "group_segment_fixed_size", "next_free_sgpr")


def kernels(path):
    text = open(path).read()
    text = re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", text))
    text = re.sub(r"Header=BB\d+_", "Header=BB_", text)      # (loop comments carry the function index too)
    out = {}
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n(.*?)^\t\.end_amdhsa_kernel", text, re.M | re.S):
        name, desc = m.group(1), m.group(2)
        body = re.search(r"^%s:.*?^\.Lfunc_end:" % re.escape(name), text, re.M | re.S)
        fig = {k: re.search(r"\.amdhsa_%s (\S+)" % k, desc).group(1) for k in FIGURES}
        out[name] = (body.group(0) if body else None, desc, fig)
    return out


def main(a_path, b_path, resources):
    a, b = kernels(a_path), kernels(b_path)
    print(f"kernels: {len(a)} / {len(b)}; only in the first: {sorted(set(a) - set(b))}; only in the second: {sorted(set(b) - set(a))}")
    same, moved, sgpr = 0, [], []
    for name in sorted(set(a) & set(b)):
        if resources:
            fa, fb = ({k: v for k, v in f.items() if k != "next_free_sgpr"} for f in (a[name][2], b[name][2]))
            (moved.append((name, fa, fb)) if fa != fb else None)
            same += fa == fb
            if a[name][2]["next_free_sgpr"] != b[name][2]["next_free_sgpr"]:
                sgpr.append(f"{name}: {a[name][2]['next_free_sgpr']} -> {b[name][2]['next_free_sgpr']}")
        else:
            same += a[name][:2] == b[name][:2] and a[name][0] is not None
            (moved.append(name) if a[name][:2] != b[name][:2] or a[name][0] is None else None)
    print(f"{'same VGPR / AGPR offset / scratch / LDS figures' if resources else 'byte-identical body and descriptor'}: {same} of {len(set(a) & set(b))}")
    for m in moved:
        print("DIFFERS", m)
    if resources:
        print(f"SGPR count moved in {len(sgpr)} kernels" + "".join("\n  " + s for s in sgpr))
    return 0 if not moved and set(a) == set(b) else 1


if __name__ == "__main__":
    args = [x for x in sys.argv[1:] if x != "--resources"]
    sys.exit(main(args[0], args[1], "--resources" in sys.argv))
