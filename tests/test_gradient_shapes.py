"""cafe_score_gradient (csrc/gradient.hip) at the smallest shapes at which each of its kernels can go wrong.

Tree: a cherry (A, B), a polytomy of 7 leaves (C..I: the product kernel takes 6 factors per launch), a clade with an
interior child ((J, K), L) and a leaf under the root (M); two lambda classes.  (M, R) in PAIRS: M in {15, 16, 63, 64, 65}
-- either side of the scan's 8-row blocks, the leaf filter's 32-column tiles and 64-row blocks, the GEMM's 16-deep K step
and 64-row tile -- with R below and above M.  Families: counts 0 and M at leaves under a 3-tap error model (taps fall
outside [0, M]), every leaf at M, duplicates.  Models: base with lambda = mu; gamma K = 3 with the error model and death
rates at rho = lambda / mu = 0.25; base with the error model and death rates at rho = 4; both root rules.  Column counts
1, 127, 128, 129 and 300 distinct families; a workspace_limit that forces three column batches; one saturated branch;
mus == lambdas against the unset call.

Reference and bound are test_gradient_gpu's: gradient_ref.reverse, |got - ref| <= 1e-12 + 1e-10 c |ref|.  Here c = 1e5: the
largest cancellation factor the reference reports on these inputs is 24990 (rho = 4: one family's d lnL / d mu passes close
to zero; 694 for the gamma configuration, 14 for the base one, 4822 over the column counts), rounded up to a power of ten
(measured on the CPU; test_the_reference_reports_the_cancellation_the_bound_assumes asserts that it lies in (1e4, 1e5]).
gradient_ref.close holds every entry to its OWN factor, which is at most that: most entries are checked at 1e-10 times a
factor below 100.

The CPU tests say what the GPU tests can see: four deliberately wrong passes of the reference (beta's second scan run
causally, the shift S dropped, the sum taken from i = 0 with Ft at i, the root weight not restricted under MAX) are each
told from the right one, by more than 100 x the bound, on every input set."""
import functools

import numpy as np
import pytest

import gradient_ref as GR
import marginal_ref as MR
from cafexp_amd import problem as P
from cafexp_amd.gamma_rates import discrete_gamma
from test_per_family_shapes import THREE_TAPS

C_BOUND = 1e5
kBN = 128
TREE = "(((A:3,B:5):4,(C:2,D:6,E:1,F:2,G:3,H:4,I:2):3,((J:2,K:3):2,L:4):1):5,M:7);"
LAMBDA_TREE = "(((A:1,B:1):1,(C:2,D:2,E:2,F:1,G:1,H:2,I:2):2,((J:1,K:2):2,L:1):1):1,M:2);"
SPECIES = list("ABCDEFGHIJKLM")
PAIRS = [(15, 12), (15, 20), (16, 14), (16, 40), (63, 50), (63, 70), (64, 40), (64, 129), (65, 60), (65, 80)]
LAMBDAS = np.array([0.02, 0.012])
CONFIGS = {
    "base": dict(model="base", err=False, mus=None),
    "gamma_err_rho_0.25": dict(model="gamma", err=True, mus=LAMBDAS * 4),
    "base_err_rho_4": dict(model="base", err=True, mus=LAMBDAS / 4),
}


def _rows(M, n, seed):
    rng = np.random.default_rng(seed)
    top = max(2, min(M, 12))
    counts = rng.integers(0, top + 1, size=(n, len(SPECIES))).astype(np.int32)
    if n >= 8:
        counts[0] = 1
        counts[1] = M                                        # every leaf at M: the tap above M falls outside
        counts[2] = [M, M - 1, M, M, M - 2, M, M - 1, M, M, M - 1, M, M, M - 2]
        counts[3] = [0, 0, 1, 0, 2, 0, 1, 0, 0, 1, 0, 0, 1]  # a cherry at 0: the tap below 0 falls outside
        counts[4] = counts[2]                                # duplicates
        counts[5] = counts[0]
    return counts


def _problem(M, R, n=24, seed=0, err=False, distinct=False):
    counts = _rows(M, n, seed + 7 * M + R)
    if distinct:
        counts = np.unique(np.random.default_rng(seed).integers(0, min(M, 12) + 1, size=(4 * n, len(SPECIES))).astype(np.int32), axis=0)[:n]
        assert len(counts) == n
    return P.build_problem(P.parse_newick(TREE), SPECIES, ["f%d" % i for i in range(n)], counts,
                           lambda_tree=P.parse_newick(LAMBDA_TREE, lambda_tree=True), root_filter=False,
                           max_family_size=M, max_root_family_size=R, n_deviations=3 if err else 0)


def _prior(R):
    w = 1.0 / np.arange(1, R + 1)                            # not uniform: the arg max is not the likelihood's alone
    return (w / w.sum()).astype(np.float32)


def _params(pb, cfg):
    pr = P.Params(lambdas=LAMBDAS.copy(), prior=_prior(pb.max_root_family_size))
    if cfg["model"] == "gamma":
        pr.cat_probs, pr.multipliers = discrete_gamma(3, 0.7)
    if cfg["err"]:
        pr.error_model = P.error_model_table(THREE_TAPS, pb.max_family_size)
    return pr


@functools.lru_cache(maxsize=None)
def _pair_case(M, R, config, rule):
    cfg = CONFIGS[config]
    pb = _problem(M, R, err=cfg["err"])
    pr = _params(pb, cfg)
    return pb, pr, cfg["mus"], GR.reverse(pb, pr, cfg["mus"], rule)


COLUMNS = [1, 127, 128, 129, 300]


@functools.lru_cache(maxsize=None)
def _column_case(n, rule="max"):
    cfg = CONFIGS["gamma_err_rho_0.25"]
    pb = _problem(40, 30, n=n, seed=n, err=True, distinct=True)
    pr = _params(pb, cfg)
    return pb, pr, cfg["mus"], GR.reverse(pb, pr, cfg["mus"], rule)


# ---------------------------------------------------------------------------------------------------- CPU
def test_the_tree_and_the_pairs_are_what_the_docstring_says():
    pb = _problem(40, 30)
    ch, root = MR.children_of(pb), MR.root_of(pb)
    leaf = lambda v: pb.leaf_taxon[v] >= 0
    inner = [v for v in range(pb.n_nodes) if not leaf(v)]
    assert any(len(ch[v]) == 2 and all(leaf(c) for c in ch[v]) for v in inner)                  # a cherry
    assert any(leaf(c) for c in ch[root])                                                       # a leaf under the root
    assert any(sum(1 for c in ch[v] if leaf(c)) == 7 for v in inner)                            # 7 > 6 factors per product launch
    assert any(v != root and any(not leaf(c) for c in ch[v]) for v in inner)                    # an interior child below the root's children
    assert pb.n_lambdas == 2 and set(pb.lambda_index) == {0, 1}
    assert {M for M, R in PAIRS} == {15, 16, 63, 64, 65}
    for M in (15, 16, 63, 64, 65):
        assert any(R < m for m, R in PAIRS if m == M) and any(R > m for m, R in PAIRS if m == M)
    for M, R in PAIRS:
        c = _problem(M, R, err=True).counts
        assert (c == 0).any() and (c == M).any() and len(np.unique(c, axis=0)) < len(c)
    em = P.error_model_table(THREE_TAPS, 15)
    assert em.shape == (16, 3) and em[15, 2] > 0                                                # the tap above M carries weight


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_the_reference_reports_the_cancellation_the_bound_assumes(config):
    worst = max(GR.worst_cancellation(_pair_case(M, R, config, rule)[3]) for M, R in PAIRS for rule in ("max", "sum"))
    print("%s: largest cancellation factor over the pairs %.1f" % (config, worst))
    assert worst <= C_BOUND
    if config == "base_err_rho_4":
        assert C_BOUND / 10 < worst
    if config == "gamma_err_rho_0.25":
        cols = max(GR.worst_cancellation(_column_case(n)[3]) for n in COLUMNS)
        print("largest cancellation factor over the column counts %.1f" % cols)
        assert cols <= C_BOUND


def _told_apart(mut, ref):
    big = False
    for key in GR.KEYS:
        if key in ref:
            ok = ~np.isnan(ref[key])
            big = big or bool(np.max(np.abs(mut[key][ok] - ref[key][ok]) / (1e-12 + 1e-10 * C_BOUND * np.abs(ref[key][ok]))) > 100)
    return big


@pytest.mark.parametrize("M,R", PAIRS)
def test_the_inputs_tell_a_wrong_pass_from_a_right_one(M, R):
    for config in sorted(CONFIGS):
        for rule in ("max", "sum"):
            pb, pr, mus, ref = _pair_case(M, R, config, rule)
            assert not ref["failed"].any()
            for name in GR.MUTANTS:
                mut = GR.reverse(pb, pr, mus, rule, mutant=name)
                label = "%s M %d R %d %s %s" % (name, M, R, config, rule)
                if name == "root_unrestricted" and rule == "sum":
                    for key in GR.KEYS:                      # the sum rule has no restriction to drop
                        assert key not in ref or np.array_equal(mut[key], ref[key]), label
                    continue
                assert _told_apart(mut, ref), label
                with pytest.raises(AssertionError):
                    GR.close(mut, ref, C_BOUND, label)


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def capi():
    from cafexp_amd import capi as C
    C.load()
    return C


def _K(pr):
    return 1 if pr.multipliers is None else len(pr.multipliers)


def _run(capi, pb, pr, mus, rule, ref, label, **ctx_args):
    ctx = capi.Context(pb, max_categories=_K(pr), **ctx_args)
    try:
        ctx.set_death_rates(mus)
        got = ctx.score_gradient(pr, rule, alpha=0.7)
    finally:
        ctx.close()
    GR.close(got, ref, C_BOUND, label)
    ok = ref["failed"] == 0
    assert np.all(np.abs(got["family_lnl"][ok] - ref["family_lnl"][ok]) <= 1e-12 + 1e-10 * np.abs(ref["family_lnl"][ok])), label
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("M,R", PAIRS)
def test_every_pair_model_and_rule(capi, M, R, config):
    for rule in ("max", "sum"):
        pb, pr, mus, ref = _pair_case(M, R, config, rule)
        got = _run(capi, pb, pr, mus, rule, ref, "M %d R %d %s %s" % (M, R, config, rule))
        assert not got["failed"].any()
        for key in GR.KEYS:                                  # duplicate families get equal rows
            if key in got:
                assert np.array_equal(got[key][4], got[key][2]) and np.array_equal(got[key][5], got[key][0]), key


@pytest.mark.gpu
@pytest.mark.parametrize("n", COLUMNS)
def test_column_counts_around_the_tile(capi, n):
    pb, pr, mus, ref = _column_case(n)
    assert len(np.unique(pb.counts, axis=0)) == n
    _run(capi, pb, pr, mus, "max", ref, "%d distinct families" % n)


def _per_col(pb, K, n_par):
    """gradient_impl's own workspace formula: bytes per column"""
    nI = int((pb.leaf_taxon < 0).sum())
    rows = pb.matrix_size
    return (3 * nI * rows + 4 * rows + K + K * pb.n_lambdas * n_par + 3) * 8


@pytest.mark.gpu
def test_three_column_batches_change_no_bit(capi):
    pb, pr, mus, ref = _column_case(300)
    per_col = _per_col(pb, 3, 2)
    limit = kBN * per_col + per_col // 2
    assert limit // per_col // kBN * kBN == kBN and -(-300 // kBN) == 3
    want = _run(capi, pb, pr, mus, "max", ref, "one batch")
    got = _run(capi, pb, pr, mus, "max", ref, "three batches", workspace_limit=limit)
    for key in want:
        assert np.array_equal(got[key], want[key], equal_nan=True), key


@pytest.mark.gpu
@pytest.mark.parametrize("config", ["base", "gamma"])
def test_equal_death_rates_give_the_unset_derivative(capi, config):
    cfg = dict(model=config, err=True, mus=None)
    pb = _problem(40, 30, err=True)
    pr = _params(pb, cfg)
    ctx = capi.Context(pb, max_categories=_K(pr))
    try:
        for rule in ("max", "sum"):
            one = ctx.score_gradient(pr, rule, alpha=0.7)
            ctx.set_death_rates(LAMBDAS)
            both = ctx.score_gradient(pr, rule, alpha=0.7)
            ctx.set_death_rates(None)
            s, r = both["d_lambda"] + both["d_mu"], one["d_lambda"]
            # the parity tolerance, entry by entry: 1e-10 of the sums of |terms| behind the three numbers
            two, unset = GR.reverse(pb, pr, LAMBDAS, rule), GR.reverse(pb, pr, None, rule)
            room = (two["cancel_d_lambda"] * np.abs(two["d_lambda"]) + two["cancel_d_mu"] * np.abs(two["d_mu"])
                    + unset["cancel_d_lambda"] * np.abs(unset["d_lambda"]))
            print("%s %s: worst |d_lambda + d_mu - unset| / bound %.3g" % (config, rule, np.max(np.abs(s - r) / (1e-12 + 1e-10 * room))))
            assert np.all(np.abs(s - r) <= 1e-12 + 1e-10 * room), rule
            assert np.array_equal(both["family_lnl"], one["family_lnl"])      # mus == lambdas: the lambda = mu bits
            if config == "gamma":
                room = two["cancel_d_multiplier"] * np.abs(two["d_multiplier"]) + unset["cancel_d_multiplier"] * np.abs(unset["d_multiplier"])
                assert np.all(np.abs(both["d_multiplier"] - one["d_multiplier"]) <= 1e-12 + 1e-10 * room)
    finally:
        ctx.close()


SATURATED_TREE = "((A:12,B:1):1,C:2);"
SATURATED_LAMBDA_TREE = "((A:2,B:1):1,C:1);"


def _saturated_case():
    rng = np.random.default_rng(3)
    counts = rng.integers(0, 9, size=(24, 3)).astype(np.int32)
    counts[::2, :2] = 0                                      # A = B = 0: possible under an extinct parent; every other family fails
    counts[:, 2] = np.maximum(counts[:, 2], 1)
    pb = P.build_problem(P.parse_newick(SATURATED_TREE), ["A", "B", "C"], ["f%d" % i for i in range(24)], counts,
                         lambda_tree=P.parse_newick(SATURATED_LAMBDA_TREE, lambda_tree=True), root_filter=False,
                         max_family_size=40, max_root_family_size=30)
    pr = P.Params(lambdas=np.array([0.02, 0.1]), prior=_prior(30))        # lambda_2 t = 1.2 on A's branch: saturated
    return pb, pr, (counts[:, 0] == 0) & (counts[:, 1] == 0)


def test_the_saturated_case_is_one():
    pb, pr, possible = _saturated_case()
    a, b = GR.alpha_beta(0.1, 0.1, 12.0)
    assert GR.is_zero(a, b) and not GR.is_zero(*GR.alpha_beta(0.02, 0.02, 2.0))
    assert sorted(pb.lambda_index[pb.leaf_taxon >= 0]).count(1) == 1 and (pb.lambda_index == 1).sum() == 1
    ref = GR.reverse(pb, pr, None, "sum")
    assert np.array_equal(ref["failed"] == 0, possible) and 8 <= possible.sum() <= 16


@pytest.mark.gpu
def test_a_saturated_branch_contributes_exactly_zero(capi):
    pb, pr, possible = _saturated_case()
    for rule in ("max", "sum"):
        ref = GR.reverse(pb, pr, None, rule)
        got = _run(capi, pb, pr, None, rule, ref, "saturated %s" % rule)
        assert np.array_equal(got["failed"] == 0, possible)
        assert np.all(got["d_lambda"][possible, 1] == 0.0) and np.all(got["d_lambda"][possible, 0] != 0.0)
        assert np.all(np.isnan(got["d_lambda"][~possible])) and np.all(np.isnan(got["family_lnl"][~possible]))
