"""cafe_score_per_family (family_lambda.hip) away from the mammals table: every instantiation of the per-family kernel
(E = 2 .. 32 columns per lane) either side of every switch of launch_family_lambda's ladder, both n_rows rules (R + 1
under the root, M + 1 elsewhere) at wide E, row counts that end on, one past and one short of a 16-row LDS block, trees
that are not binary, 3-tap and 5-tap error models at counts 0, 1, M - 1 and M, the bench's own shape (100 taxa, order
751) and the batch cut at a wide order.

Every value is compared with two references at REL = 1e-10 (test_lambda_per_family._close: infinities must match
exactly): the CPU oracle, oracle.score_base(pb, pr, fast=True, per_family=True), one call per distinct lambda vector,
and the scorer path on the same context, ctx.score(pr, per_family=True)["family_lnl"].  Every family has its own
lambdas, all families in one call."""
import dataclasses

import numpy as np
import pytest

from cafexp_amd import problem as P, synth
from helpers import _explicit_problem
from test_gpu_parity import _random_problem
from test_lambda_per_family import _close

WIDTHS = [2, 4, 6, 8, 10, 12, 14, 16, 20, 24, 28, 32]
# 3 .. 33: row counts around a 16-row block; then either side of every change of the columns per lane (n <= 64 * E)
ORDERS = [3, 16, 17, 33, 128, 129, 256, 257, 384, 385, 512, 513, 640, 641, 768, 769, 896, 897, 1024, 1025, 1280, 1281,
          1536, 1537, 1792, 1793, 2047, 2048]
TREE3 = "((A:7.25,B:23.904):61.337,C:9.75);"
LAMBDAS = [0.0011, 0.002, 0.0051, 0.0034]


def width(n):
    """E of launch_family_lambda's width dispatch (for_lane_width) at matrix order n."""
    return next(E for E in WIDTHS if n <= 64 * E)


def sizes(n):
    """(M, R) with max(M, R) + 1 == n: M > R at even n, R > M at odd n (R = M = 2 at n = 3)."""
    return (n - 1, n // 2) if n % 2 == 0 else (n * 4 // 5, n - 1)


def families(n):
    """Four kinds, cut to M where the order is small: tiny counts, counts near n / 4, a zero count at one leaf, counts in
    the forties."""
    M = sizes(n)[0]
    q = n // 4
    rows = [{"A": 3, "B": 5, "C": 2}, {"A": q, "B": q - q // 12, "C": q + q // 16}, {"A": 0, "B": 1, "C": 1}, {"A": 40, "B": 44, "C": 39}]
    return [{s: min(c, M) for s, c in r.items()} for r in rows]


@pytest.fixture(scope="module")
def capi(oracle):
    from cafexp_amd import capi as C
    C.load()
    oracle.set_threads(min(16, oracle.host_cpu_share()))
    return C


def _check(capi, oracle, pb, prior, lambdas, error_model=None, fam=None):
    """score_per_family of the families `fam` (all of pb's by default), family fam[i] under lambdas[i], against the oracle
    and against the scorer path of the same context: one evaluation of each per distinct lambda vector.  Returns the
    per-family values."""
    fam = np.arange(pb.n_families) if fam is None else np.asarray(fam)
    lam = np.asarray(lambdas, dtype=np.float64).reshape(len(fam), -1)
    assert lam.shape[1] == pb.n_lambdas and len(np.unique(lam, axis=0)) >= 3
    sub = dataclasses.replace(pb, counts=np.ascontiguousarray(pb.counts[fam]), family_ids=[pb.family_ids[i] for i in fam])
    ctx = capi.Context(pb)
    try:
        got = ctx.score_per_family(P.Params(lambdas=np.ones(pb.n_lambdas), prior=prior, error_model=error_model), fam, lam)
        want_oracle, want_scorer = np.empty(len(fam)), np.empty(len(fam))
        for vec in np.unique(lam, axis=0):
            sel = np.all(lam == vec, axis=1)
            pr = P.Params(lambdas=vec.copy(), prior=prior, error_model=error_model)
            want_oracle[sel] = oracle.score_base(sub, pr, fast=True, per_family=True)[1][sel]
            want_scorer[sel] = ctx.score(pr, per_family=True)[1]["family_lnl"][fam[sel]]
    finally:
        ctx.close()
    print("against the oracle: ", end="")
    _close(got, want_oracle)
    print("against the scorer: ", end="")
    _close(got, want_scorer)
    return got


# ---------------------------------------------------------------------------------------------------- CPU
def test_the_orders_reach_every_instantiation_and_row_tail():
    assert {width(n) for n in ORDERS} == set(WIDTHS)
    for lo, hi in zip(WIDTHS, WIDTHS[1:]):                   # both sides of every switch: the last order of E, the first of the next
        assert 64 * lo in ORDERS and width(64 * lo) == lo
        assert 64 * lo + 1 in ORDERS and width(64 * lo + 1) == hi
    assert 2048 in ORDERS and width(2048) == 32              # the library's limit
    rows_under_root, rows_elsewhere = set(), set()
    for n in ORDERS:
        M, R = sizes(n)
        assert max(M, R) + 1 == n
        assert all(0 <= c <= M for r in families(n) for c in r.values())
        rows_under_root.add((R + 1) % 16)                    # n_rows of the branches under the root: C's and the one above (A, B)
        rows_elsewhere.add((M + 1) % 16)                     # n_rows of A's and B's branches
    # the flush of the last block of parked rows: a row count on a block's end, one past it, one short of it
    assert 0 in rows_elsewhere and {1, 15} <= rows_under_root
    assert min(ORDERS) < 16                                  # fewer rows than one block
    for E in (20, 24, 28, 32):                               # both n_rows rules at the widest instantiations: M > R and R > M
        assert {sizes(n)[0] > sizes(n)[1] for n in ORDERS if width(n) == E} == {True, False}


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("n", ORDERS)
def test_every_width_against_the_oracle_and_the_scorer(capi, oracle, n):
    """a. One family of each kind, each under its own lambda, at matrix order n."""
    M, R = sizes(n)
    pb = _explicit_problem(TREE3, families(n), M, R)
    assert pb.matrix_size == n
    got = _check(capi, oracle, pb, P.prior_uniform(R), LAMBDAS)
    print("n %d E %d M %d R %d: lnL %s" % (n, width(n), M, R, got))
    assert np.isfinite(got).all()                            # a table of -inf would compare equal and check nothing


SHAPES = [
    ("(A:1.5,B:2.25,C:0.7);", None),                                                 # polytomy at the root, leaves under the root
    ("((A:1,B:1,C:2,D:0.5,E:1,F:3):2,(G:1,H:2):0.5,I:4);",                           # six leaf children, a leaf under the root
     "((A:1,B:1,C:2,D:2,E:1,F:1):2,(G:1,H:2):1,I:2);"),
    ("((((A:1,B:1):1,C:2):1,D:3):1,E:4);", "((((A:1,B:1):1,C:2):2,D:2):1,E:1);"),      # caterpillar
    ("(((A:1,B:1):1,(C:1,D:1):1):1,((E:1,F:1):1,(G:1,H:1):1):1);", None),            # balanced
    ("((A:0.0004,B:1):1,C:2);", None),                                               # t_q = 0 branch: rows s >= 1 are 0
]
SHAPE_LAMBDAS = [[0.004, 0.03], [0.011, 0.011], [0.02, 0.006], [0.033, 0.05], [0.05, 0.015]]


@pytest.mark.gpu
@pytest.mark.parametrize("M,R,prior", [(40, 30, "uniform"), (250, 299, "poisson")])
@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_tree_shapes(capi, oracle, shape, M, R, prior):
    """b. The trees of test_gpu_parity.test_tree_shapes at two orders that differ in E (41: E = 2, 300: E = 6), every family
    with its own lambdas; two shapes carry a second lambda through a lambda tree."""
    newick, lambda_newick = SHAPES[shape]
    assert width(max(M, R) + 1) == {40: 2, 250: 6}[M]
    pb = _random_problem(np.random.default_rng(5 + shape), newick, 70, M, R, 12)
    if lambda_newick:
        index = {nd.key(): nd.lambda_index - 1 for nd in P.parse_newick(lambda_newick, lambda_tree=True).postorder()}
        pb = dataclasses.replace(pb, lambda_index=np.array([index[k] for k in pb.node_names], dtype=np.int32), n_lambdas=2, single_lambda=False)
        assert set(pb.lambda_index) == {0, 1}
    possible = np.ones(pb.n_families, dtype=bool)
    if "A:0.0004" in newick:
        # A's matrix is e_0 in row 0 and zero below: a family is possible only with A = 0 under an extinct parent, so B = 0
        # too.  Every other family has likelihood 0 (lnL -inf, which _close wants matched exactly).
        counts = pb.counts.copy()
        counts[::2, [pb.taxa.index("A"), pb.taxa.index("B")]] = 0
        pb = dataclasses.replace(pb, counts=counts)
        possible = (counts[:, pb.taxa.index("A")] == 0) & (counts[:, pb.taxa.index("B")] == 0)
        assert possible.sum() >= 35 and (~possible).sum() >= 20
    lam = np.array([SHAPE_LAMBDAS[f % 5][:pb.n_lambdas] for f in range(pb.n_families)])
    got = _check(capi, oracle, pb, P.prior_uniform(R) if prior == "uniform" else P.prior_poisson(R, 4.0), lam)
    assert np.array_equal(np.isfinite(got), possible)


FIVE_TAPS = [[0.0, 0.0, 0.8, 0.15, 0.05], [0.0, 0.1, 0.75, 0.1, 0.05], [0.05, 0.1, 0.7, 0.1, 0.05]]
THREE_TAPS = [[0.0, 0.9, 0.1], [0.1, 0.8, 0.1]]


@pytest.mark.gpu
@pytest.mark.parametrize("taps,M,R", [(5, 40, 30), (5, 60, 70), (3, 40, 30), (3, 140, 150)])
def test_error_model_taps_at_the_ends_of_the_range(capi, oracle, taps, M, R):
    """c. The tree and the 5-tap model of test_five_tap_error_model_and_mixed_leaf_counts, and a 3-tap model: families
    whose counts are 0, 1, M - 1 and M drop the taps below 0 and above M (with R > M the columns past M exist)."""
    tree = P.parse_newick("((A:3,B:5,C:2,(D:4,E:6):3):4,(F:6,G:1):2);")
    species = ["A", "B", "C", "D", "E", "F", "G"]
    counts = np.random.default_rng(11 + taps + M).integers(0, 15, size=(64, 7)).astype(np.int32)
    counts[0] = 0
    counts[1] = [1, 0, 2, 0, 1, 0, 3]
    counts[2] = [0, 1, 1, 0, 0, 1, 0]
    counts[3] = M
    counts[4] = [M, M - 1, M, M - 1, M - 2, M, M - 1]
    counts[5] = M - 1
    counts[6] = [M - 3, M - 1, M, M - 2, M, M - 1, M - 4]
    pb = P.build_problem(tree, species, ["f%d" % i for i in range(64)], counts, root_filter=False, n_deviations=taps,
                         max_family_size=M, max_root_family_size=R)
    for c in (0, 1, M - 1, M):
        assert (pb.counts == c).any(), c
    em = P.error_model_table(FIVE_TAPS if taps == 5 else THREE_TAPS, M)
    assert em.shape == (M + 1, taps) and em[M, -1] > 0         # the tap that falls above M carries weight
    lam = np.array([0.01, 0.03, 0.021, 0.044])[np.arange(64) % 4]
    got = _check(capi, oracle, pb, P.prior_uniform(R), lam, error_model=em)
    assert np.isfinite(got[:7]).all()


@pytest.mark.gpu
def test_bench_shape(capi, oracle):
    """d. The bench's table shape: synth.make_problem on 100 taxa, largest count 600, matrix order 751 (E = 12); eight
    families, family 0 (which sets the order) among them, each under its own lambda."""
    pb, _ = synth.make_problem(n_taxa=100, n_families=3000, max_count=600)
    assert pb.n_taxa == 100 and pb.n_nodes == 199 and pb.matrix_size == 751 and width(751) == 12
    assert pb.counts[0].max() == 600
    fam = np.array([0, 1, 2, 17, 400, 1111, 2222, pb.n_families - 1])
    got = _check(capi, oracle, pb, P.prior_uniform(pb.max_root_family_size), np.linspace(0.0008, 0.0043, len(fam)), fam=fam)
    assert np.isfinite(got).all()


@pytest.mark.gpu
def test_batch_cut_at_a_wide_order(capi, monkeypatch):
    """e. Order 1281 (E = 24): one family per batch and the automatic batch give the same bits."""
    n = 1281
    assert width(n) >= 20
    M, R = sizes(n)
    rows = families(n) + [{"A": 7, "B": 0, "C": 3}, {"A": 120, "B": 111, "C": 130}, {"A": 1, "B": 1, "C": 1}]
    pb = _explicit_problem(TREE3, rows, M, R)
    pr = P.Params(lambdas=np.array([1.0]), prior=P.prior_uniform(R))
    fam = np.array([6, 0, 1, 2, 3, 4, 5, 1, 6])
    lam = np.array(LAMBDAS)[np.arange(len(fam)) % 4]
    results = []
    for cap in (1, 0):
        monkeypatch.setenv("CAFE_PER_FAMILY_BATCH", str(cap))
        ctx = capi.Context(pb)
        try:
            results.append(ctx.score_per_family(pr, fam, lam))
        finally:
            ctx.close()
    assert np.isfinite(results[0]).all()
    assert np.array_equal(results[0], results[1])
