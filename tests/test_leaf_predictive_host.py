"""The arithmetic behind `cafexp_hip --leaf-predictive` -- the two-sided p of a cell, Holm's adjustment over the finite cells, the
order of the outliers, the summary per species -- in its own CPU-only test program (cafexp_amd/host/leaf_predictive_tests.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cafexp_amd", "host")


def test_the_report_arithmetic_unit_tests_pass():
    mk = subprocess.run(["make", "-s", "-C", HOST, "leaf_predictive_tests"], capture_output=True, text=True)
    assert mk.returncode == 0, mk.stdout + mk.stderr
    out = subprocess.run([os.path.join(HOST, "leaf_predictive_tests")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failures" in out.stdout
