"""What `cafexp_hip --branch-change` does on the host -- the cell text, the per-branch sums and counts of the summary, what the
root and a failed family contribute, the two files as written -- in its own CPU-only test program
(cafexp_amd/host/branch_change_tests.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cafexp_amd", "host")


def test_the_branch_change_report_unit_tests_pass():
    mk = subprocess.run(["make", "-s", "-C", HOST, "branch_change_tests"], capture_output=True, text=True)
    assert mk.returncode == 0, mk.stdout + mk.stderr
    out = subprocess.run([os.path.join(HOST, "branch_change_tests")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failures" in out.stdout
