"""The edges of the sum rule's reductions and of cafe_root_posterior's two kernels, on small synthetic tables:
  R in {1, 15, 16, 17, 250}        the 16 row segments of the sum-rule K4 and of the per-column kernel;
  R in {63, 64, 65}                the 64 lanes of the per-family root kernel;
  distinct families in {1, 15, 16, 17, 127, 128, 129, 300}   the 16 families of a workgroup, the 128-column tiles of the row kernel;
  duplicated families              the multiplicities in total and n_used;
  three column chunks              family_lnl, total, mean, mode, log_evidence bit for bit those of one chunk;
  one sharded context over [0]     the setter applied to its shard, equal to the plain context.
Reference: tests/root_rule_ref.py fed the matrices the call itself built; |got - ref| <= 1e-12 + 1e-10 |ref| (total: floor
1e-12 n_families); mode exact unless the reference's two best masses lie within 1e-9, at most 5 % of a case's families."""
import numpy as np
import pytest

import marginal_ref as MR
import root_rule_ref as RR
from cafexp_amd import problem as P
from cafexp_amd.gamma_rates import discrete_gamma
from test_gpu_parity import _random_problem
from test_root_posterior_gpu import within_total
from test_root_rule_gpu import capi, same_bits, within  # noqa: F401 (capi: the fixture)
from test_root_rule_model import MAX_EXCUSED, TIE, prior_one_over_s

pytestmark = pytest.mark.gpu

TREE4 = "((A:3,B:5):4,(C:2,D:6):3);"
TREE8 = "(((A:1,B:1):1,(C:1,D:1):1):1,((E:1,F:1):1,(G:1,H:1):1):1);"
R_EDGES = (1, 15, 16, 17, 63, 64, 65, 250)
F_EDGES = (1, 15, 16, 17, 127, 128, 129, 300)


def table(n_distinct, n_repeats, M, R, hi, seed):
    """n_distinct different rows of four counts below `hi`, then the first n_repeats of them again"""
    rng = np.random.default_rng(seed)
    rows, seen = [], set()
    while len(rows) < n_distinct:
        r = tuple(int(x) for x in rng.integers(0, hi, size=4))
        if r not in seen and sum(r) > 0:
            seen.add(r)
            rows.append(r)
    counts = np.array(rows + rows[:n_repeats], dtype=np.int32)
    tree = P.parse_newick(TREE4)
    return P.build_problem(tree, ["A", "B", "C", "D"], ["f%d" % i for i in range(len(counts))], counts, root_filter=False,
                           max_family_size=M, max_root_family_size=R)


def params(R, gamma):
    pr = P.Params(lambdas=np.array([0.02]), prior=prior_one_over_s(R))
    if gamma:
        pr.cat_probs, pr.multipliers = discrete_gamma(2, 0.7)
    return pr


def check(capi, pb, pr, label, per_family):
    K = 1 if pr.multipliers is None else len(pr.multipliers)
    ctx = capi.Context(pb, max_categories=K)
    try:
        ctx.set_root_rule("sum")
        value, fam = ctx.score(pr, alpha=0.7, per_family=True)
        L = RR.root_vectors(pb, pr, MR.context_matrices(ctx, pb, K))
        rule, post = RR.sum_rule(pr, L), RR.root_posterior(pr, L)
        assert not post["failed"].any()
        within(fam["family_lnl"], rule["family_lnl"], label + " family_lnl")
        within(value, RR.neg_lnl(rule["family_lnl"]), label + " -lnL")
        if K > 1:
            within(fam["category_likelihood"], rule["category_likelihood"], label + " category_likelihood")
        if per_family:
            fams = np.arange(pb.n_families)
            within(ctx.score_per_family(pr, fams, np.full(pb.n_families, pr.lambdas[0])), fam["family_lnl"], label + " per-family entry")
        got = ctx.root_posterior(pr, alpha=0.7)
        assert same_bits(got["log_evidence"], fam["family_lnl"])
        assert got["n_used"] == pb.n_families and not got["failed"].any()
        within(got["mean"], post["mean"], label + " mean")
        within_total(got["total"], post["total"], pb.n_families, label + " total")
        within_total(got["total"].sum(), got["n_used"], pb.n_families, label + " sum of total")
        if K > 1:
            within(got["category_posterior"], post["category_posterior"], label + " category_posterior")
        differ, excused = got["mode"] != post["mode"], post["mode_gap"] <= TIE
        assert not np.any(differ & ~excused), label
        assert excused.mean() <= MAX_EXCUSED, label         # (the reference alone)
    finally:
        ctx.close()


@pytest.mark.parametrize("R", R_EDGES)
def test_every_edge_of_the_root_range(capi, R):
    pb = table(20, 3, 20, R, 9, seed=R)
    assert pb.matrix_size == max(20, R) + 1
    for gamma in (False, True):
        check(capi, pb, params(R, gamma), "R %d %s" % (R, "gamma" if gamma else "base"), per_family=not gamma)


@pytest.mark.parametrize("n", F_EDGES)
def test_every_edge_of_the_family_count(capi, n):
    pb = table(n, min(n, 3), 12, 10, 9, seed=100 + n)
    for gamma in (False, True):
        check(capi, pb, params(10, gamma), "%d families %s" % (n, "gamma" if gamma else "base"), per_family=False)


def test_three_column_chunks_change_no_bit(capi):
    """test_gpu_parity.py's chunked case -- 600 families, five 128-column tiles, gamma K = 2 -- under the sum rule: two chunks
    of two tiles and a narrower last one, or five of one tile, give the bits of one chunk."""
    pb = _random_problem(np.random.default_rng(11), TREE8, 600, 60, 50, 25)
    pr = P.Params(lambdas=np.array([0.01]), prior=prior_one_over_s(50))
    pr.cat_probs, pr.multipliers = discrete_gamma(2, 2.0)
    one = capi.Context(pb, max_categories=2)
    one.set_root_rule("sum")
    v1, r1 = one.score(pr, alpha=2.0, per_family=True)
    p1 = one.root_posterior(pr, alpha=2.0)
    assert one.stats()["n_chunks"] == 1
    one.close()
    seen = set()
    for tiles in (1, 2):
        many = capi.Context(pb, max_categories=2, workspace_limit=5 * 2 * 80 * 8 * 128 * tiles + 1)
        many.set_root_rule("sum")
        v2, r2 = many.score(pr, alpha=2.0, per_family=True)
        seen.add(many.stats()["n_chunks"])
        assert same_bits(v1, v2)
        for key in r1:
            assert same_bits(r1[key], r2[key]), key
        p2 = many.root_posterior(pr, alpha=2.0)
        assert many.stats()["n_chunks"] >= 3
        for key in ("total", "mean", "mode", "log_evidence", "category_posterior", "failed"):
            assert same_bits(p1[key], p2[key]), key
        assert p1["n_used"] == p2["n_used"] == 600
        many.close()
    assert 3 in seen, seen


def test_a_sharded_context_follows_its_shards_rule(capi):
    pb = table(40, 5, 12, 10, 9, seed=7)
    pr = params(10, True)
    one = capi.Context(pb, max_categories=2)
    one.set_root_rule("sum")
    v1, r1 = one.score(pr, alpha=0.7, per_family=True)
    one.close()
    sh = capi.Sharded(pb, [0], max_categories=2)
    try:
        assert sh.size == 1
        before = sh.score(pr, alpha=0.7)
        sh.set_root_rule("sum")
        assert sh.shard(0).root_rule() == "sum"
        v2, r2 = sh.score(pr, alpha=0.7, per_family=True)
        assert v2 < before
        within(v2, v1, "sharded -lnL")                      # (another family order inside the shard: the sum's rounding only)
        for key in r1:
            assert np.array_equal(r1[key], r2[key]), key
    finally:
        sh.close()
