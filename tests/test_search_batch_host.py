"""The look-ahead search on the CPU: cafexp_amd/host/search_batch_tests (mock scorers, no HIP library) -- the batched optimizer
feeds nm_search the sequential optimizer's (point, value) sequence bit for bit on every objective, dimension and batch size, and
stays within one batch for the first simplex, one per iteration and one per shrink."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cafexp_amd", "host")


def test_the_program_passes():
    exe = os.path.join(HOST, "search_batch_tests")
    subprocess.check_call(["make", "-s", "-C", HOST, "search_batch_tests"])      # (incremental: never a stale program)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout
    assert "search_batch_tests: all passed" in out.stdout
    for name in ("log-quadratic (a)", "Rosenbrock (b)", "infinite at vertex 1 (c)"):
        assert sum(line.startswith(name) for line in out.stdout.splitlines()) >= 2, name
