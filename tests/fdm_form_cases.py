"""Boundary lists of the per-direction form tests (tests/test_fdm_form_cpu.py, tests/test_fdm_form_gpu.py): (label, component, value) with face labels 0/1 = x, 2/3 = y,
4/5 = z, and the split mask (x, y, z) each must get: a direction is split iff every component has the same condition at both of its ends (and the line is uniform)."""
from common import BC_3D

# components disagree within a direction (the list of tests/test_fdm_u_gpu.py)
MIXED_3D = [(0, 0, 0.0), (1, 0, -1e-5), (2, 1, 0.0), (3, 1, -1e-5), (4, 2, 0.0), (2, 0, 2e-6), (5, 1, 0.0)]
COLUMN = [(0, 0, 0.0), (1, 0, 0.0), (2, 1, 0.0), (3, 1, 0.0), (4, 2, 0.0)]          # the consolidation column: rollers on the sides, held at the bottom, free top
X_ONE_SIDED = [(0, 0, 0.0)] + BC_3D[2:]
Y_ONE_SIDED = BC_3D[:2] + [(2, 1, 0.0)] + BC_3D[4:]

FORM_CASES = {
    "column": ((1, 1, 0), COLUMN),
    "x_one_sided": ((0, 1, 1), X_ONE_SIDED),
    "y_one_sided": ((1, 0, 1), Y_ONE_SIDED),
    "only_y": ((0, 1, 0), [(0, 0, 0.0), (2, 1, 0.0), (3, 1, 0.0), (4, 2, 0.0)]),
    "only_z": ((0, 0, 1), [(0, 0, 0.0), (2, 1, 0.0), (4, 2, 0.0), (5, 2, 0.0)]),
    "mixed": ((1, 0, 0), MIXED_3D),
    "low_faces": ((0, 0, 0), [(0, 0, 0.0), (2, 1, 0.0), (4, 2, 0.0)]),
}
BOXES = [((3, 4, 5), 2), ((5, 3, 4), 1)]          # (the Q1 box: even node counts, no centre node, in x)
GRADED = ((4, 3, 5), 2, (1.0, 0.0, -0.7), (0, 1, 0))      # cells, degree, grading, mask: BC_3D on a box graded in x and z
