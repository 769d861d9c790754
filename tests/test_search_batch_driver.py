"""`cafexp_hip --search-batch 4` against the same run without it, at one seed: the look-ahead search scores its points through
cafe_score_batch and must leave the sequential search's trajectory -- every file under -o byte for byte, every stdout line but
the JSON one, and in the JSON line the iterations, scorer_calls and every value -- with fewer device round trips than points
consumed.  Also the option's refusals at argument checking (no GPU needed)."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cafexp_amd", "host", "cafexp_hip")
DATA = os.path.join(ROOT, "tests", "golden", "data")
MAMMALS = ["-t", os.path.join(DATA, "mammals_tree.txt"), "-i", os.path.join(DATA, "mammals_1500.txt")]
SYNTH20 = ["-t", os.path.join(DATA, "synth20_tree.txt"), "-i", os.path.join(DATA, "synth20_families.txt")]

CASES = {
    "mammals_base": MAMMALS,
    "mammals_k3": MAMMALS + ["-k", "3"],
    "mammals_estimate_mu": MAMMALS + ["--estimate-mu"],
    "synth20_lambda_tree": SYNTH20 + ["-y", os.path.join(DATA, "synth20_lambda_tree.txt")],
}


def run(args, out_dir):
    os.makedirs(out_dir)                                     # (the driver writes into an existing directory)
    p = subprocess.run([EXE, "-s", "7", "-o", str(out_dir)] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr + p.stdout
    lines = p.stdout.splitlines()
    files = {name: open(os.path.join(out_dir, name), "rb").read() for name in sorted(os.listdir(out_dir))}
    return lines[:-1], json.loads(lines[-1]), files


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_look_ahead_search_leaves_what_the_sequential_search_leaves(tmp_path, name):
    lines0, json0, files0 = run(CASES[name], tmp_path / "sequential")
    lines1, json1, files1 = run(CASES[name] + ["--search-batch", "4"], tmp_path / "batched")
    assert files0 and sorted(files0) == sorted(files1)
    for f in files0:
        assert files0[f] == files1[f], f
    assert lines0 == lines1
    s0, s1 = json0.pop("search"), json1.pop("search")
    print(name, "sequential", s0, "batched", s1)
    assert "batches" not in s0 and "points_scored" not in s0
    assert s1["iterations"] == s0["iterations"] and s1["scorer_calls"] == s0["scorer_calls"] and s1["score"] == s0["score"]
    assert 0 < s1["batches"] < s1["scorer_calls"] and s1["points_scored"] >= s1["batches"]
    for d in (json0, json1):                                  # wall times of the final calls
        for key in [k for k in d if "seconds" in k or k.endswith("_ms") or k.endswith("_s")]:
            d.pop(key)
    assert json0 == json1


@pytest.mark.gpu
def test_an_estimated_error_model_runs_the_loop_and_says_so(tmp_path):
    args = MAMMALS + ["-e", "--limit", "300"]
    lines0, json0, files0 = run(args, tmp_path / "sequential")
    lines1, json1, files1 = run(args + ["--search-batch", "4"], tmp_path / "batched")
    notice = [ln for ln in lines1 if ln.startswith("--search-batch:")]
    assert len(notice) == 1 and "one call each" in notice[0]
    assert [ln for ln in lines1 if ln not in notice] == lines0
    for f in files0:
        assert files0[f] == files1[f], f
    assert json1["search"]["scorer_calls"] == json0["search"]["scorer_calls"] and json1["search"]["score"] == json0["search"]["score"]


@pytest.mark.parametrize("extra,why", [
    (["--search-batch", "1"], "at least 2"),
    (["--search-batch", "0"], "at least 2"),
    (["--search-batch", "33"], "must not exceed 32"),
    (["--search-batch", "11", "-k", "3"], "must not exceed 32"),
    (["--search-batch", "4", "--gpus", "2"], "--gpus"),
    (["--search-batch", "4", "-b"], "-b is not supported"),
    (["--search-batch", "4", "--simulate", "10", "-l", "0.01"], "--simulate is not supported"),
])
def test_refusals_at_argument_checking(tmp_path, extra, why):
    out = tmp_path / "out"
    p = subprocess.run([EXE, "-o", str(out)] + MAMMALS + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert p.returncode == 1, (p.returncode, p.stderr)
    assert "--search-batch" in p.stderr and why in p.stderr, p.stderr
    assert not out.exists() and p.stdout == ""
