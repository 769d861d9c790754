"""What `cafexp_hip --missing / --mask-cells` does on the host -- reading a table with unknown cells, masking cells by (family,
species), sizes and root filter from the observed cells, the imputed-counts arithmetic -- in its own CPU-only test program
(cafexp_amd/host/missing_cells_tests.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cafexp_amd", "host")


def test_the_missing_cell_unit_tests_pass():
    mk = subprocess.run(["make", "-s", "-C", HOST, "missing_cells_tests"], capture_output=True, text=True)
    assert mk.returncode == 0, mk.stdout + mk.stderr
    out = subprocess.run([os.path.join(HOST, "missing_cells_tests")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failures" in out.stdout
