"""The gain model's host side on the CPU: cafexp_amd/host/gain_tests (mock scorers, no HIP library) -- the table of distinct
families and its weights, the search vector, the conditional objective as lnL_absent -> 0-, the nested search and the refusals
(cafexp_amd/host/gain_tests.cpp)."""
import os
import subprocess

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cafexp_amd", "host")


def test_gain_host_logic():
    mk = subprocess.run(["make", "-s", "-C", HOST, "gain_tests"], capture_output=True, text=True)      # (incremental: never a stale program)
    assert mk.returncode == 0, mk.stderr[-2000:]
    out = subprocess.run([os.path.join(HOST, "gain_tests")], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "gain_tests: all passed" in out.stdout
