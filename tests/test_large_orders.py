"""The HIP path at matrix orders 752 .. 2048 -- every order a family table with a largest count up to 1637 reaches, and
the library's limit (bd_matrix_max_order() = 2048).  One large family sets the order of a whole table, so these orders send
every kernel of every call down variants that smaller tables never run:
  * K1 (bd_matrix.hip): a lane owns E columns, E = 14, 16, 20, 24, 28, 32 above 768 (E > 16 masks the columns past the matrix
    with selects instead of the (1-a)^2 zero trick).  The scorer's two-pool launch sizes E by n columns, the single-pool
    launch of the k-major layout by n - 1: the orders either side of every switch run through both.
  * K2 / the planner (K tiles 8 deep: up to 256 K tiles and 128 extent blocks per matrix), K3 / K4 over R up to 2046,
    K5 and cafe_root_max.
Values are compared with the reference (tests/golden/ref_large_order.json) and with the oracle (its O(N^2) matrix build,
pinned to the reference at these orders by tests/test_large_order_golden.py) at the tolerances of test_gpu_parity.py;
the work-skipping and scheduling switches must not change a bit."""
import dataclasses
import json
import math
import os

import numpy as np
import pytest

from cafexp_amd import problem as P, synth
from helpers import _explicit_problem, case_from_args, rel_err
from test_large_order_golden import check_matrix

pytestmark = pytest.mark.gpu

SCORE_TOL = 1e-10
VEC_TOL = 5e-11
WIDTHS = [2, 4, 6, 8, 10, 12, 14, 16, 20, 24, 28, 32]
# either side of every change of K1's columns per lane above 751, for n columns (row-major, two-pool) and n - 1 (k-major)
ORDERS = [768, 769, 770, 896, 897, 898, 1024, 1025, 1026, 1280, 1281, 1536, 1537, 1792, 1793, 2047, 2048]


def k1_width(cols):
    """E of K1's width dispatch (for_lane_width) for a launch over `cols` owned columns."""
    return next(E for E in WIDTHS if cols <= 64 * E)


@pytest.fixture(scope="module")
def capi(oracle):
    from cafexp_amd import capi as C
    C.load()
    oracle.set_threads(min(16, oracle.host_cpu_share()))
    return C


@pytest.fixture(scope="module")
def large():
    with open(os.path.join(os.path.dirname(__file__), "golden", "ref_large_order.json")) as f:
        return json.load(f)


def _check_vs_oracle(got, want, cols=None):
    """test_matrix_build_vs_oracle's assertions: row 0 = e_0, zero rows stay zero, entries above 1e-290 to VEC_TOL, the
    deep-underflow rule, every entry in [0, 1]."""
    cols = got.shape[1] if cols is None else cols
    got, want = got[:, :cols], want[:, :cols]
    assert np.array_equal(got[0], want[0])
    if not want[1:].any():                                   # saturated / t_q = 0: rows s >= 1 are exactly 0
        assert not got[1:].any()
    big = want > 1e-290
    worst = float((np.abs(got - want)[big] / want[big]).max(initial=0.0))
    assert worst <= VEC_TOL, worst
    assert got[~big].max(initial=0.0) <= 1e-280 and want[got <= 1e-290].max(initial=0.0) <= 1e-280
    assert got.min() >= 0.0 and got.max() <= 1.0
    return worst


def test_the_orders_reach_every_wide_k1_instantiation():
    for cols_of in (lambda n: n, lambda n: n - 1):
        assert {k1_width(cols_of(n)) for n in ORDERS} >= {14, 16, 20, 24, 28, 32}
        for E in (12, 14, 16, 20, 24, 28):                   # both sides of every switch
            assert any(k1_width(cols_of(n)) == E for n in ORDERS) and any(k1_width(cols_of(n)) == WIDTHS[WIDTHS.index(E) + 1] for n in ORDERS)


# ------------------------------------------------------------------ K1, single-pool launch (cafe_build_matrices)
# (lambda, t): a long and a short branch, a saturated one (a > 1/2) and one whose length quantizes to t_q = 0
BATCH = [(0.0011, 23.904), (0.0051, 7.25), (0.9, 5.0), (0.002, 0.0004)]


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("n", ORDERS)
def test_single_pool_matrices_against_the_oracle(capi, oracle, n, layout):
    """layout 0: row-major (n columns per launch); layout 1: the k-major layout through reversibility (n - 1 columns)."""
    got = capi.build_matrices(n, [l for l, _ in BATCH], [t for _, t in BATCH], layout=layout)
    for i, (lam, t) in enumerate(BATCH):
        want = oracle.build_matrix(n, lam, t, fast=True)
        _check_vs_oracle(got[i], want)
        if i >= 2:
            assert not want[1:].any() and got[i][0, 0] == 1.0 and not got[i][1:].any()


@pytest.mark.parametrize("layout", [0, 1])
def test_single_pool_matrices_against_the_reference(capi, large, layout):
    for e in large["matrices"]:
        got = capi.build_matrices(e["n"], [e["lambda"]], [e["t"]], layout=layout)[0]
        worst = check_matrix(got, e, VEC_TOL)
        print("n %d lambda %.6g t %g layout %d: worst relative error %.3g" % (e["n"], e["lambda"], e["t"], layout, worst))


def test_order_above_the_limit_is_an_argument_error(capi):
    with pytest.raises(capi.CafeError, match="code 1"):         # CAFE_ERR_ARGUMENT
        capi.build_matrices(2049, [0.002], [10.0])


# ------------------------------------------------------------------ K1, two-pool launch (the scorer's)
FAMS = [{"A": 3, "B": 5, "C": 2}, {"A": 300, "B": 280, "C": 310}, {"A": 0, "B": 1, "C": 1}, {"A": 40, "B": 44, "C": 39}]


@pytest.mark.parametrize("n", ORDERS)
def test_two_pool_matrices_and_scores_against_the_oracle(capi, oracle, n):
    """A scorer call builds its leaf (row-major) and interior (k-major) matrices in one launch with n columns per lane set.
    Explicit sizes give the order: M = n - 1 (R < M) at even n, R = n - 1 (M < R) at odd n."""
    M, R = (n - 1, n // 2) if n % 2 == 0 else (n * 4 // 5, n - 1)
    pb = _explicit_problem("((A:7.25,B:23.904):61.337,C:9.75);", FAMS, M, R)
    assert pb.matrix_size == n
    probs, mult = oracle.discrete_gamma(2, 0.8)
    pr = P.Params(lambdas=np.array([0.002]), prior=P.prior_uniform(R), multipliers=mult, cat_probs=probs)
    ctx = capi.Context(pb, max_categories=2)
    v, res = ctx.score(pr, alpha=0.8, per_family=True)
    want_v, want_cat, _ = oracle.score_gamma(pb, pr, fast=True, per_family=True)
    assert rel_err(v, want_v) <= SCORE_TOL, (v, want_v)
    big = want_cat > 1e-290
    assert (np.abs(res["category_likelihood"] - want_cat)[big] / want_cat[big]).max() <= VEC_TOL
    kinds = set()
    for node in range(pb.n_nodes):
        if pb.parent[node] < 0:
            continue
        leaf = pb.leaf_taxon[node] >= 0
        kinds.add(leaf)
        for k in (0, 1):
            want = oracle.build_matrix(n, 0.002 * float(mult[k]), float(pb.branch_length[node]), fast=True)
            _check_vs_oracle(ctx.matrix(node, k), want, cols=None if leaf else M + 1)   # interior: contraction sizes 0..M
    assert kinds == {True, False}
    ctx.close()


@pytest.mark.parametrize("i", range(5))
def test_two_pool_matrices_against_the_reference(capi, large, i):
    """The fixture's (lambda, t) on a leaf branch and an interior branch of a scorer call whose sizes are those of the table
    the fixture's order stands for (1025: M = 982, R = 1024; 2047: M = 1964, R = 2046)."""
    e = large["matrices"][i]
    t = e["t"]
    pb = _explicit_problem("((A:%r,B:1.5):%r,C:2.5);" % (t, t), FAMS, e["M"], e["R"])
    assert pb.matrix_size == e["n"]
    ctx = capi.Context(pb)
    ctx.score(P.Params(lambdas=np.array([e["lambda"]]), prior=P.prior_uniform(e["R"])))
    names = {nm: v for v, nm in enumerate(pb.node_names)}
    leaf = names["A"]
    interior = int(pb.parent[leaf])
    assert pb.parent[interior] >= 0 and pb.branch_length[interior] == t
    w0 = check_matrix(ctx.matrix(leaf), e, VEC_TOL)
    w1 = check_matrix(ctx.matrix(interior), e, VEC_TOL, cols=e["M"] + 1)
    print("two-pool n %d lambda %.6g t %g: worst relative error leaf %.3g interior %.3g" % (e["n"], e["lambda"], t, w0, w1))
    ctx.close()


# ------------------------------------------------------------------ scores against the reference
@pytest.mark.parametrize("name", ["large6_gamma_k4", "large6_base", "large6_multilambda_err", "huge6_base"])
def test_scores_against_the_reference(capi, oracle, large, name):
    e = large["scores"][name]
    pb, pr, alpha = case_from_args(e["args"], oracle)
    K = len(pr.multipliers) if pr.multipliers is not None else 1
    for subtree_dedup in (True, False):
        ctx = capi.Context(pb, max_categories=K, subtree_dedup=subtree_dedup)
        v = ctx.score(pr, alpha=alpha)
        assert rel_err(v, e["neg_lnl"]) <= SCORE_TOL, (v, e["neg_lnl"])
        res = ctx.family_results(K if pr.multipliers is not None else 0)
        if pr.multipliers is not None:
            assert np.abs(res["category_likelihood"].ravel() / np.array(e["category_likelihood"]) - 1).max() <= VEC_TOL
            assert np.abs(res["family_likelihood"] / np.array(e["family_likelihood"]).reshape(-1, K)[:, 0] - 1).max() <= VEC_TOL
        else:
            assert np.abs(res["family_lnl"] / np.array(e["family_lnl"]) - 1).max() <= SCORE_TOL
        ctx.close()


# ------------------------------------------------------------------ scores against the oracle at three orders
def _sample(pb, idx):
    return dataclasses.replace(pb, counts=np.ascontiguousarray(pb.counts[idx]), family_ids=[pb.family_ids[i] for i in idx])


CASES = {
    # name: (max count, families, model, sizes (M, R) or None)
    "n1126_base": (900, 2000, "base", None),
    "n1126_gamma_k8": (900, 600, "gamma8", None),
    "n1126_m_above_r_gamma_k2": (900, 800, "gamma2", (1400, 1000)),
    "n1626_multilambda_err": (1300, 1000, "err", None),
    "n2047_base": (1637, 400, "base", None),
}


@pytest.mark.parametrize("name", list(CASES))
def test_scores_against_the_oracle(capi, oracle, name):
    mx, F, model, sizes = CASES[name]
    pb, _ = synth.make_problem(n_taxa=8, n_families=F, max_count=mx, lam_sim=0.002, seed=mx + F, root_cap=200,
                               lambda_clade_min=2 if model == "err" else 0, n_deviations=3 if model == "err" else 0)
    if sizes:
        pb = dataclasses.replace(pb, max_family_size=sizes[0], max_root_family_size=sizes[1])
        assert pb.max_family_size > pb.max_root_family_size
    R = pb.max_root_family_size
    assert pb.matrix_size == {900: 1126, 1300: 1626, 1637: 2047}[mx] if not sizes else pb.matrix_size == sizes[0] + 1
    pr = P.Params(lambdas=np.array([0.0021] if model != "err" else [0.0021, 0.0034]), prior=P.prior_uniform(R))
    alpha, K = 1.0, 1
    if model.startswith("gamma"):
        K = int(model[5:])
        alpha = 1.3
        pr.cat_probs, pr.multipliers = oracle.discrete_gamma(K, alpha)
    if model == "err":
        assert pb.n_lambdas == 2
        pr.error_model = P.error_model_table(P.default_error_model(pb.max_family_size)[:1] + [[0.05, 0.9, 0.05]], pb.max_family_size)
    ctx = capi.Context(pb, max_categories=K)
    v, res = ctx.score(pr, alpha=alpha, per_family=True)
    assert math.isfinite(v)
    idx = np.unique(np.r_[0, 1, 2, np.arange(3, pb.n_families, max(1, pb.n_families // 10)), pb.n_families - 1])
    sub = _sample(pb, idx)
    if K > 1:
        _, cat, fam = oracle.score_gamma(sub, pr, fast=True, per_family=True)
        big = cat > 1e-290
        assert (np.abs(res["category_likelihood"][idx] - cat)[big] / cat[big]).max() <= VEC_TOL
        assert np.abs(res["family_likelihood"][idx] / fam - 1).max() <= VEC_TOL
    else:
        _, fam = oracle.score_base(sub, pr, fast=True, per_family=True)
        assert np.abs(res["family_lnl"][idx] / fam - 1).max() <= SCORE_TOL
    ctx.close()


# ------------------------------------------------------------------ the same bits whatever the schedule
def _bits(r1, r2):
    return r1.keys() == r2.keys() and all(np.array_equal(r1[k], r2[k]) for k in r1)


def test_schedules_and_switches_have_the_same_bits_at_1126(capi, oracle, monkeypatch):
    """One context called with wide, narrow and again wide extents (lambda large, small, large) against a fresh context per
    call, CAFE_NO_KSKIP, CAFE_NO_GROUPS, graph replay, every forced tile height and a chunked workspace."""
    pb, _ = synth.make_problem(n_taxa=8, n_families=800, max_count=900, lam_sim=0.002, seed=77, root_cap=200)
    assert pb.matrix_size == 1126
    K, alpha = 4, 0.9
    probs, mult = oracle.discrete_gamma(K, alpha)
    R = pb.max_root_family_size
    calls = [P.Params(lambdas=np.array([lam]), prior=P.prior_uniform(R), multipliers=mult, cat_probs=probs) for lam in (0.003, 0.0004, 0.003)]
    ctx = capi.Context(pb, max_categories=K)
    base = [ctx.score(pr, alpha=alpha, per_family=True) for pr in calls]
    assert base[0][0] == base[2][0] and _bits(base[0][1], base[2][1])
    assert rel_err(base[1][0], oracle.score_gamma(pb, calls[1], fast=True)) <= SCORE_TOL

    def check(other, label):
        for pr, (v, r) in zip(calls, base):
            v2, r2 = other.score(pr, alpha=alpha, per_family=True)
            assert v2 == v and _bits(r, r2), label

    for pr, (v, r) in zip(calls, base):
        fresh = capi.Context(pb, max_categories=K)
        v2, r2 = fresh.score(pr, alpha=alpha, per_family=True)
        assert v2 == v and _bits(r, r2), "fresh"
        fresh.close()
    for env in ("CAFE_NO_KSKIP", "CAFE_NO_GROUPS"):
        monkeypatch.setenv(env, "1")
        other = capi.Context(pb, max_categories=K)
        monkeypatch.delenv(env)
        check(other, env)
        other.close()
    g = capi.Context(pb, max_categories=K)
    g.set_graphs(True)
    check(g, "graphs")
    g.close()
    for mi in (2, 3, 4, 5, 6, 7, 8, 9, 0):
        ctx.force_tile(mi)
        check(ctx, "tile %d" % mi)
    # a chunked workspace: room for two column tiles of a guessed number of panels (rows_pad = 1152 at M = 1080, R = 1125)
    chunks = set()
    for n_panels in (3, 4, 5, 6):
        try:
            many = capi.Context(pb, max_categories=K, workspace_limit=n_panels * K * 1152 * 8 * 128 * 2 + 1)
        except capi.CafeError:
            continue
        chunks.add(many.stats()["n_chunks"])
        check(many, "chunks %d" % many.stats()["n_chunks"])
        many.close()
    assert max(chunks) >= 2, chunks
    ctx.close()


# ------------------------------------------------------------------ K5 and cafe_root_max at N = 1126
def test_root_max_and_reconstruct_at_1126(capi, oracle):
    from test_reconstruct import _near_tie_only
    pb, _ = synth.make_problem(n_taxa=8, n_families=512, max_count=900, lam_sim=0.002, seed=5, root_cap=200)
    assert pb.matrix_size == 1126
    lam = np.array([0.002])
    jmax = min(pb.max_family_size, pb.max_root_family_size)
    rp = np.zeros(jmax + 1, dtype=np.float32)
    rp[:pb.max_root_family_size] = P.prior_uniform(pb.max_root_family_size)[:jmax + 1]
    ctx = capi.Context(pb)
    st = ctx.reconstruct(lam, rp)[0]
    rm = ctx.root_max(lam)
    idx = np.array([0, 1, 2, 100, 311, 511])
    sub = _sample(pb, idx)
    want = oracle.reconstruct(sub, lam, rp, fast=True)[0]
    pr = P.Params(lambdas=lam, prior=P.prior_uniform(pb.max_root_family_size))
    _near_tie_only(sub, pr, rp, st[idx], want, 1.0)
    assert st[0].max() > 751                                  # the large family's states reach past the old orders
    assert np.max(np.abs(rm[idx] / oracle.root_max(sub, lam, fast=True) - 1)) < 1e-10
    ctx.close()


# ------------------------------------------------------------------ the limit
def test_a_table_past_the_limit_is_rejected_and_the_limit_itself_works(capi, oracle):
    tree = P.parse_newick("((A:1,B:2):1,C:3);")
    counts = np.array([[1638, 1600, 1620], [1, 2, 1]], dtype=np.int32)
    pb = P.build_problem(tree, ["A", "B", "C"], ["f0", "f1"], counts)
    assert pb.matrix_size == 2049
    with pytest.raises(capi.CafeError, match=r"matrix order 2049 exceeds 2048"):
        capi.Context(pb)
    # the process goes on: N = 2048 through explicit sizes is accepted and meets the oracle
    pb = dataclasses.replace(pb, max_family_size=2047, max_root_family_size=2047)
    assert pb.matrix_size == 2048
    pr = P.Params(lambdas=np.array([0.002]), prior=P.prior_uniform(2047))
    ctx = capi.Context(pb)
    v, res = ctx.score(pr, per_family=True)
    assert math.isfinite(v)
    _, fam = oracle.score_base(pb, pr, fast=True, per_family=True)
    assert np.abs(res["family_lnl"] / fam - 1).max() <= SCORE_TOL
    ctx.close()
