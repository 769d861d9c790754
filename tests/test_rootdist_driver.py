"""cafexp_hip --root-sum, --estimate-rootdist and --rootdist-probs end to end, on 300 families simulated (numpy, fixed seed)
down the six-taxon tree of tests/bd_lm_ref.py from root sizes 1 + Poisson(4).

  --root-sum             the printed -lnL is the binding's sum-rule score at the printed lambda; the max-rule run of the same
                         command says nothing of a rule and prints the binding's max-rule score;
  --estimate-rootdist 3  -lnL per round does not increase by more than n_families 2^-23: the EM step is exact in doubles, and
                         rounding the prior to the float the ABI takes moves each family's Z by at most 2^-24 relative; the
                         written distribution sums to 1 within R 2^-24; --rootdist-probs on that file reproduces the last
                         round's -lnL at the last round's lambda to 1e-10 relative;
  --standard-errors --root-sum   recomputed from the binding's CAFE_ROOT_SUM scores at 1e-8 (test_standard_errors_driver.py);
  the two refused combinations print their messages and exit 1."""
import json
import os
import subprocess

import numpy as np
import pytest

import bd_lm_ref as BL
from cafexp_amd import problem as P
from test_standard_errors_driver import DRIVER, _parse

pytestmark = pytest.mark.gpu

SPECIES = ["A", "B", "C", "D", "E", "F"]
N_FAMILIES, LAMBDA_SIM, ORDER_SIM = 300, 0.01, 61


def simulated_counts():
    tree = P.parse_newick(BL.NEWICK)
    nodes = tree.postorder()
    rng = np.random.default_rng(20261019)
    mats = {}
    rows = []
    for _ in range(N_FAMILIES):
        size = {id(tree): 1 + int(rng.poisson(4.0))}
        for n in reversed(nodes):                            # parents before children
            if n.parent is None:
                continue
            if n.length not in mats:
                m = BL.matrix(ORDER_SIM, LAMBDA_SIM, LAMBDA_SIM, n.length)
                mats[n.length] = m / m.sum(axis=1, keepdims=True)
            size[id(n)] = int(rng.choice(ORDER_SIM, p=mats[n.length][size[id(n.parent)]]))
        leaf = {n.name: size[id(n)] for n in nodes if n.is_leaf}
        rows.append([leaf[s] for s in SPECIES])
    return np.array(rows, dtype=np.int32)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """(tree file, family file, the binding's problem) of the simulated table"""
    d = tmp_path_factory.mktemp("rootdist")
    counts = simulated_counts()
    tree_path, fam_path = str(d / "tree.txt"), str(d / "families.txt")
    with open(tree_path, "w") as f:
        f.write(BL.NEWICK + "\n")
    with open(fam_path, "w") as f:
        f.write("Desc\tFamily ID\t" + "\t".join(SPECIES) + "\n")
        for i, r in enumerate(counts):
            f.write("(null)\tfam%d\t" % i + "\t".join(str(int(x)) for x in r) + "\n")
    ids = ["fam%d" % i for i in range(len(counts))]
    pb = P.build_problem(P.parse_newick(BL.NEWICK), SPECIES, ids, counts)
    assert 250 <= pb.n_families <= N_FAMILIES
    return tree_path, fam_path, pb


def run(data, out, *extra, ok=True):
    assert os.path.exists(DRIVER), "cafexp_hip missing: run __graft_entry__.build()"
    r = subprocess.run([DRIVER, "-t", data[0], "-i", data[1], "-s", "7", "-o", str(out)] + list(extra), capture_output=True, text=True, timeout=300)
    if not ok:
        return r
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def binding_score(pb, js, rule, prior=None):
    from cafexp_amd import capi
    pr = P.Params(lambdas=np.array(js["lambda"]), prior=P.prior_uniform(pb.max_root_family_size) if prior is None else prior)
    ctx = capi.Context(pb)
    try:
        ctx.set_root_rule(rule)
        return ctx.score(pr)
    finally:
        ctx.close()


def test_root_sum_searches_the_sum_rule_and_leaves_the_max_rule_alone(data, tmp_path):
    pb = data[2]
    js = run(data, tmp_path, "--root-sum")
    assert js["root_rule"] == "sum" and js["n_families"] == pb.n_families
    want = binding_score(pb, js, "sum")
    assert abs(js["neg_lnl"] - want) <= 1e-12 * abs(want), (js["neg_lnl"], want)
    assert any(ln.startswith("Root rule: sum") for ln in open(os.path.join(str(tmp_path), "Base_results.txt")))
    mx = run(data, tmp_path)
    assert "root_rule" not in mx
    want = binding_score(pb, mx, "max")
    assert abs(mx["neg_lnl"] - want) <= 1e-12 * abs(want)
    assert not any("Root rule" in ln for ln in open(os.path.join(str(tmp_path), "Base_results.txt")))
    assert mx["neg_lnl"] > js["neg_lnl"]


def test_estimate_rootdist_rounds_and_the_file_it_writes(data, tmp_path):
    pb = data[2]
    R = pb.max_root_family_size
    js = run(data, tmp_path, "--estimate-rootdist", "3")
    rounds = js["rootdist"]["rounds"]
    print("rounds:", rounds)
    assert js["root_rule"] == "sum" and 2 <= len(rounds) <= 4
    for a, b in zip(rounds, rounds[1:]):
        assert b <= a + pb.n_families * 2.0 ** -23, rounds
    assert rounds[1] < rounds[0] - 1.0                       # (the uniform start is far from the simulated root sizes)
    assert js["neg_lnl"] == rounds[-1]
    lines = [ln for ln in open(os.path.join(str(tmp_path), "Base_results.txt")) if ln.startswith("Root distribution round")]
    assert len(lines) == len(rounds) and all("Lambda:" in ln for ln in lines)
    path = os.path.join(str(tmp_path), "Base_root_distribution.txt")
    rows = [ln.split("\t") for ln in open(path).read().splitlines()]
    assert [int(r[0]) for r in rows] == list(range(1, R + 1))
    probs = np.array([float(r[1]) for r in rows])
    assert abs(probs.sum() - 1.0) <= R * 2.0 ** -24 and np.all(probs >= 0)
    assert np.array_equal(probs, probs.astype(np.float32).astype(np.float64))       # the floats the ABI took
    os.makedirs(str(tmp_path / "again"))
    again = run(data, tmp_path / "again","--root-sum", "--rootdist-probs", path, "-l", repr(js["lambda"][0]))
    assert abs(again["neg_lnl"] - rounds[-1]) <= 1e-10 * abs(rounds[-1]), (again["neg_lnl"], rounds[-1])
    want = binding_score(pb, js, "sum", prior=probs.astype(np.float32))
    assert abs(want - rounds[-1]) <= 1e-10 * abs(want)


def test_standard_errors_differentiate_what_was_searched(data, tmp_path):
    from cafexp_amd import capi
    pb = data[2]
    js = run(data, tmp_path, "--root-sum", "--standard-errors")
    names, tab, corr, total = _parse(os.path.join(str(tmp_path), "Base_standard_errors.txt"))
    assert names == ["Lambda"]
    pr = P.Params(lambdas=np.array(js["lambda"]), prior=P.prior_uniform(pb.max_root_family_size))
    ctx = capi.Context(pb)
    try:
        g = ctx.score_gradient(pr, "sum")
        g_max = ctx.score_gradient(pr, "max")
    finally:
        ctx.close()
    S = g["d_lambda"][:, :1]
    want_se = np.sqrt(np.diag(np.linalg.inv(S.T @ S)))
    other = np.sqrt(np.diag(np.linalg.inv(g_max["d_lambda"][:, :1].T @ g_max["d_lambda"][:, :1])))
    print("SE", tab[:, 1], "numpy (sum)", want_se, "numpy (max)", other)
    assert np.all(np.abs(tab[:, 1] - want_se) <= 1e-8 * want_se)
    assert np.allclose(total, S.sum(axis=0), rtol=1e-8, atol=1e-8 * np.sqrt(np.trace(S.T @ S)))
    assert abs(other[0] - want_se[0]) > 1e-6 * want_se[0]   # (the max rule's scores are other numbers)


@pytest.mark.parametrize("extra,word", [(["-b"], "-b"), (["--gpus", "2"], "--gpus")])
def test_the_refused_combinations(data, tmp_path, extra, word):
    r = run(data, tmp_path, "--estimate-rootdist", *extra, ok=False)
    assert r.returncode == 1 and "--estimate-rootdist" in r.stderr and word in r.stderr
