"""What the per-cell coefficient fields share (csrc/cell_field.hpp), without a GPU: the classification by layers, cell order -> lattice order with its two refusals, the
field state of one and two components, layers by cell centres, inheritance through coarse cells - through tests/cell_field_check.cpp, a stand-alone program built with
the address and undefined-behaviour sanitizers and run directly (its exit code names the check that failed)."""
import subprocess

from common import build_sanitized_check


def test_cell_field_module_under_the_sanitizers(tmp_path):
    run = subprocess.run([build_sanitized_check(tmp_path, "cell_field_check")], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "cell_field_check ok", (run.returncode, run.stderr)
