"""bench.py's own contract: a plain run times --steps steps of the headline call and nothing else, and --dump-outputs writes
what the last timed step returned (-lnL and the per-family results) as float64 .npy files, at most bench.DUMP_BYTES in
all, so that two builds can be compared value for value on the same seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Results:
    """Stands in for a context: cafe_family_results of a call over F families and K categories."""

    def __init__(self, F, K):
        self.F, self.K = F, K

    def family_results(self, K):
        assert K == self.K
        res = {"family_lnl": -np.arange(self.F, dtype=np.float64), "failed": np.zeros(self.F, dtype=np.int32)}
        if K:
            res["category_likelihood"] = np.tile(np.arange(self.F, dtype=np.float64)[:, None], (1, K))
            res["family_likelihood"] = np.arange(self.F, dtype=np.float64)
        return res


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d) if f.endswith(".npy")}


def test_dump_keeps_a_fixed_sample_of_the_families_under_the_size_cap(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 4 << 20)
    got = []
    for i in range(2):
        d = str(tmp_path / str(i))
        bench.dump_outputs(d, 123.5, _Results(100000, 8), 8)
        assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 4 << 20
        got.append(_load(d))
    a = got[0]
    assert sorted(a) == ["category_likelihood", "failed", "family_index", "family_likelihood", "family_lnl", "neg_lnl"]
    assert all(v.dtype == np.float64 for v in a.values()) and a["neg_lnl"].tolist() == [123.5]
    idx = a["family_index"]
    assert 0 < len(idx) < 100000 and np.all(np.diff(idx) > 0)
    assert np.array_equal(a["family_lnl"], -idx) and np.array_equal(a["category_likelihood"][:, 3], idx)
    assert all(np.array_equal(a[k], got[1][k]) for k in a)                 # the same sample every run
    # below the cap every family; a rejected call (+inf) has no per-family results
    bench.dump_outputs(str(tmp_path / "small"), 1.0, _Results(1000, 0), 1)
    assert sorted(_load(str(tmp_path / "small"))) == ["failed", "family_lnl", "neg_lnl"]
    bench.dump_outputs(str(tmp_path / "inf"), float("inf"), None, 8)
    assert sorted(_load(str(tmp_path / "inf"))) == ["neg_lnl"]


@pytest.mark.gpu
def test_plain_run_dumps_what_its_last_timed_step_returned(tmp_path):
    common = ["--families", "3000", "--taxa", "20", "--max-count", "250", "--categories", "4", "--steps", "3", "--warmup", "1"]
    runs = []
    for i in range(2):
        d = str(tmp_path / str(i))
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dump-outputs", d] + common,
                           capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
        runs.append((json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]), _load(d)))
    line, a = runs[0]
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["unit"] == "families/s"
    assert not {"cpu_baseline", "parity_sample", "one_column_per_family", "other_configs"} & set(line)     # --full only
    assert sorted(a) == ["category_likelihood", "failed", "family_likelihood", "family_lnl", "neg_lnl"]
    assert all(v.dtype == np.float64 for v in a.values())
    assert a["neg_lnl"].tolist() == [line["neg_lnl"]] and np.isfinite(line["neg_lnl"])
    assert a["family_lnl"].shape == (3000,) and a["category_likelihood"].shape == (3000, 4) and not a["failed"].any()
    assert all(np.array_equal(a[k], runs[1][1][k]) for k in a)               # same arguments, same inputs, same bits
