"""Fixtures FROM THE REFERENCE at matrix orders above 751, up to the largest a family table can reach.  The library accepts
orders up to bd_matrix_max_order() = 2048; under the reference's size rules (user_data.cpp:45-46) a largest count m gives
N = max(m + max(50, m / 5), rint(1.25 m)) + 1, so m = 900 -> N = 1126 and m = 1637 -> N = 2047.
tests/golden/ref_large_order.json was printed by the compiled reference (oracle/_ref/ref_harness, generator
tests/golden/make_large_order_golden.py):
  * rows 1, 2, M, R, N-1 and the diagonal (every 64th entry + the band edges) and a sample of band-edge / deep-tail
    entries of transition matrices at N = 1025 (the first order where the scorer's two-pool K1 launch uses 20 columns per
    lane) and N = 2047
  * on a 6-taxon table with a family at 900 (N = 1126): gamma K = 4 per family and category, the base model, a lambda tree
    (two rates) + a 3-tap error model; on a 6-taxon table with a family at 1637 (N = 2047): the base model
These CPU tests pin the oracle to them (the -m gpu tests in tests/test_large_orders.py compare the HIP path with both)."""
import json
import math
import os

import numpy as np
import pytest

from cafexp_amd import problem as P
from helpers import case_from_args, rel_err

TIGHT = 1e-12          # oracle.bd_prob (the reference's own log-space sum) against the reference
CONV = 2e-11           # the O(N^2) recurrence the device uses against the reference (as at 751)
SCORES = ["large6_gamma_k4", "large6_base", "large6_multilambda_err", "huge6_base"]


@pytest.fixture(scope="module")
def large():
    with open(os.path.join(os.path.dirname(__file__), "golden", "ref_large_order.json")) as f:
        return json.load(f)


def fixture_points(e):
    """(s, c, value) of a fixture matrix: the thinned rows and diagonal and the sample."""
    return ([(s, s, v) for s, v in e["diag"]] + [(int(r), c, v) for r, row in e["rows"].items() for c, v in row]
            + [tuple(x) for x in e["sample"]])


def check_matrix(got, e, tol, cols=None):
    """got: an N x N matrix (only columns < cols are compared when cols is given); e: a fixture matrix entry.  Entries above
    1e-290 to `tol` relative, the deep tail (below that the log-space sum itself loses digits) flushes to <= 1e-280."""
    cols = e["n"] if cols is None else cols
    pts = np.array([p for p in fixture_points(e) if p[1] < cols])
    g, exp = got[pts[:, 0].astype(int), pts[:, 1].astype(int)], pts[:, 2]
    big = exp > 1e-290
    worst = float((np.abs(g - exp)[big] / exp[big]).max(initial=0.0))
    assert g[~big].max(initial=0.0) <= 1e-280 and exp[g <= 1e-290].max(initial=0.0) <= 1e-280
    assert worst <= tol, worst
    return worst


def test_fixture_covers_the_large_orders(large):
    assert sorted({m["n"] for m in large["matrices"]}) == [1025, 2047]
    for m in large["matrices"]:
        assert max(m["M"], m["R"]) + 1 == m["n"] and m["diag"][-1][0] == m["n"] - 1
        assert {int(r) for r in m["rows"]} == {1, 2, m["M"], m["R"], m["n"] - 1}
        assert all(row[-1][0] == m["n"] - 1 and len(row) >= m["n"] // 64 for row in m["rows"].values())
        tail = [v for _, _, v in m["sample"] if 0 < v < 1e-280]
        assert tail, "the sample reaches the deep tail"
    sizes = {name: (e["max_family_size"], e["max_root_family_size"]) for name, e in large["scores"].items()}
    assert sizes == {"large6_gamma_k4": (1080, 1125), "large6_base": (1080, 1125), "large6_multilambda_err": (1080, 1125),
                     "huge6_base": (1964, 2046)}
    assert all(math.isfinite(e["neg_lnl"]) for e in large["scores"].values())


def test_size_rule_puts_the_limit_between_1637_and_1638():
    """user_data.cpp:45-46 through build_problem: the largest count 1637 gives N = 2047, 1638 gives N = 2049 (rint(2047.5) =
    2048, ties to even) -- the first table the library rejects (its limit is 2048)."""
    tree = P.parse_newick("((A:1,B:2):1,C:3);")
    for mx, M, R, N in [(900, 1080, 1125, 1126), (1300, 1560, 1625, 1626), (1637, 1964, 2046, 2047), (1638, 1965, 2048, 2049)]:
        counts = np.array([[mx, 3, 5], [1, 2, 1]], dtype=np.int32)
        pb = P.build_problem(tree, ["A", "B", "C"], ["f0", "f1"], counts)
        assert (pb.max_family_size, pb.max_root_family_size, pb.matrix_size) == (M, R, N), mx


@pytest.mark.parametrize("i", range(5))
def test_oracle_matrix_entries_at_large_orders(oracle, large, i):
    """Every stored entry by the reference's own O(N) sum per entry (probability.cpp:101-147)."""
    e = large["matrices"][i]
    lq, tq = oracle.quantize(e["lambda"], e["t"])
    worst = 0.0
    for s, c, v in fixture_points(e):
        got = oracle.bd_prob(lq, tq, s, c) if s > 0 else float(c == 0)
        if v > 1e-290:
            worst = max(worst, abs(got - v) / v)
        else:
            assert got <= 1e-280 and v <= 1e-280
    assert worst <= TIGHT, worst


@pytest.mark.parametrize("i", range(5))
def test_oracle_fast_matrices_at_large_orders(oracle, large, i):
    e = large["matrices"][i]
    check_matrix(oracle.build_matrix(e["n"], e["lambda"], e["t"], fast=True), e, CONV)


@pytest.mark.parametrize("name", SCORES)
def test_oracle_scores_at_large_orders(oracle, large, name):
    e = large["scores"][name]
    pb, pr, alpha = case_from_args(e["args"], oracle)
    assert (pb.n_families, pb.max_family_size, pb.max_root_family_size) == (e["n_families"], e["max_family_size"], e["max_root_family_size"])
    if pr.multipliers is not None:
        assert np.abs(pr.multipliers / np.array(e["multipliers"]) - 1).max() <= 1e-13
        v, cat, fam = oracle.score_gamma(pb, pr, fast=True, per_family=True)
        assert np.abs(cat.ravel() / np.array(e["category_likelihood"]) - 1).max() <= CONV
        assert np.abs(fam / np.array(e["family_likelihood"]).reshape(cat.shape)[:, 0] - 1).max() <= CONV
    else:
        v, fam = oracle.score_base(pb, pr, fast=True, per_family=True)
        assert np.abs(fam / np.array(e["family_lnl"]) - 1).max() <= CONV
    assert rel_err(v, e["neg_lnl"]) <= CONV, (v, e["neg_lnl"])
