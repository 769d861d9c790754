"""Separate birth and death rates on the GPU: K1's two-rate instantiation against the numpy reference (tests/bd_lm_ref.py), bit identity with
the lambda = mu path when mu = lambda, and every call that builds matrices under cafe_set_death_rates against a numpy prune on the
reference matrices.

Tolerances: matrices VEC_TOL = 5e-11 relative, the bound tests/test_gpu_parity.py holds K1 to against the oracle (the same
arithmetic, plus the one extra rounding of the k-major scaling); -lnL and root likelihoods the project's 1e-10 relative;
the marginal reconstruction |d| <= 1e-12 + 1e-10 |ref| with exact integers away from ties (tests/test_marginal_gpu.py)."""
import numpy as np
import pytest

import bd_lm_ref as R
import marginal_ref as MR
from bd_lm_ref import LAMBDAS, MUS, problem as _problem, params as _params, reference_matrices as _reference_matrices, \
    score_from_root_vectors as _score_from_root_vectors, pupko as _pupko
from cafexp_amd import problem as P

pytestmark = pytest.mark.gpu

SCORE_TOL = 1e-10


@pytest.fixture(scope="module")
def capi():
    from cafexp_amd import capi as C
    C.load()
    return C


# ------------------------------------------------------------------ matrices
_ref_cache = {}


def _reference(n, key):
    if (n, key) not in _ref_cache:
        _ref_cache[(n, key)] = R.matrix(n, *key)
    return _ref_cache[(n, key)]


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("n", R.ORDERS)
def test_two_rate_matrices_vs_numpy(capi, n, layout):
    keys = list(R.RATES.values()) + [R.SATURATED]
    got = capi.build_matrices_lm(n, [k[0] for k in keys], [k[1] for k in keys], [k[2] for k in keys], layout=layout)
    for name, key, g in zip(list(R.RATES) + ["saturated"], keys, got):
        want = _reference(n, key)
        assert np.array_equal(g[0], want[0]), name                       # row 0 = e_0
        assert g.min() >= 0.0 and g.max() <= 1.0, name
        if name == "saturated":
            assert not g[1:].any()
            continue
        assert g[1:].any(), name
        big = want > 1e-290
        worst = R.worst_rel(g, want)
        print("order %d layout %d %s: worst relative difference / VEC_TOL = %.3g" % (n, layout, name, worst / R.VEC_TOL))
        assert worst <= R.VEC_TOL, (name, worst)
        # deep-underflow entries may flush to 0 at different places in the two algorithms
        assert g[~big].max(initial=0.0) <= 1e-280 and want[g <= 1e-290].max(initial=0.0) <= 1e-280, name


def test_equal_rates_build_the_k1_matrices_bit_for_bit(capi):
    for n in (16, 129, 300):
        for layout in (0, 1):
            a = capi.build_matrices(n, [0.006335, 0.01], [68.7105, 30.0], layout=layout)
            b = capi.build_matrices_lm(n, [0.006335, 0.01], [0.006335, 0.01], [68.7105, 30.0], layout=layout)
            assert np.array_equal(a, b), (n, layout)


# K1 is one body (bd_matrix_build.h) instantiated per slot type: with mu = lambda the two instantiations must give the same bits
# at EVERY width E = 2 .. 32 columns per lane.  64 E_prev + 1 is the smallest order of a width in the row-major layout
# (columns = n); 128 / 129 and 2048 are where the k-major layout (columns = n - 1) chooses differently, 2048 the maximum.
EVERY_WIDTH = [2, 128, 129, 257, 385, 513, 641, 769, 897, 1025, 1281, 1537, 1793, 2048]


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("n", EVERY_WIDTH)
def test_equal_rates_build_the_k1_matrices_at_every_width(capi, n, layout):
    lam, t = [0.006335, 0.01, R.SATURATED[0]], [68.7105, 30.0, R.SATURATED[2]]
    a = capi.build_matrices(n, lam, t, layout=layout)
    b = capi.build_matrices_lm(n, lam, lam, t, layout=layout)
    assert a[:2, 1:].any() and not a[2, 1:].any()          # two live keys, the third saturated at mu = lambda too
    assert np.array_equal(a, b)


# ------------------------------------------------------------------ the calls of a context (problem and numpy prune: bd_lm_ref.py)
def _compare_marginal(got, ref, label):
    for key in ("mean", "p_increase", "p_decrease", "log_evidence"):
        g, r = np.asarray(got[key]), np.asarray(ref[key])
        assert np.array_equal(np.isnan(g), np.isnan(r)), (label, key)
        ok = ~np.isnan(r)
        ratio = np.abs(g[ok] - r[ok]) / (1e-12 + 1e-10 * np.abs(r[ok]))
        print("%s %s: worst |d| / bound = %.3g" % (label, key, ratio.max(initial=0.0)))
        assert np.all(ratio <= 1), (label, key, ratio.max())
    assert np.array_equal(got["failed"], ref["failed"]), label
    for key, mask in zip(("mode", "lo", "hi"), MR.excused(ref)):
        diff = np.asarray(got[key]) != np.asarray(ref[key])
        assert not np.any(diff & ~mask), (label, key, np.argwhere(diff & ~mask)[:5])


@pytest.mark.parametrize("model", ["base", "gamma", "error"])
@pytest.mark.parametrize("order", [41, 300])
def test_scorer_and_marginal_under_death_rates(capi, order, model):
    pb = _problem(order, n_dev=3 if model == "error" else 0)
    pr = _params(pb, model)
    K = 1 if pr.multipliers is None else len(pr.multipliers)
    mults = [1.0] if pr.multipliers is None else list(pr.multipliers)
    mats = _reference_matrices(pb, LAMBDAS, MUS, mults)
    ref = MR.updown(pb, pr, mats, 0.95)
    ctx = capi.Context(pb, max_categories=K)
    ctx.set_death_rates(MUS)
    got = ctx.score(pr, alpha=0.7)
    want = _score_from_root_vectors(pr, ref["root_inside"])
    print("order %d %s: -lnL gpu %.12f numpy %.12f rel %.2e" % (order, model, got, want, abs(got - want) / abs(want)))
    assert np.isfinite(want) and abs(got - want) <= SCORE_TOL * abs(want)
    assert ctx.score(pr, alpha=0.7) != pytest.approx(capi.Context(pb, max_categories=K).score(pr, alpha=0.7), rel=1e-6)   # the model is on
    for f in range(pb.n_families):
        for k in range(K):
            g, r = ctx.root_likelihoods(f, k), ref["root_inside"][f][k]
            big = r > 1e-290
            assert (np.abs(g - r)[big] / r[big]).max(initial=0.0) <= SCORE_TOL, (f, k)
            assert g[~big].max(initial=0.0) <= 1e-280
    # the matrices the call built, and their published extents (orders >= 256)
    for k in range(K):
        for v in range(pb.n_nodes):
            if pb.parent[v] < 0:
                continue
            m = ctx.matrix(v, k)
            cols = pb.matrix_size if pb.leaf_taxon[v] >= 0 else pb.max_family_size + 1       # interior: columns > M are not materialised
            assert not R.differs(m[:, :cols], mats[k][v][:, :cols], R.VEC_TOL), (k, v)
            if order >= 256:
                ext, _ = ctx.extents(v, k)
                s, c = np.nonzero(m)
                if pb.leaf_taxon[v] >= 0:
                    assert np.all(ext[c, 0] <= s) and np.all(s <= ext[c, 1]), (k, v)
                else:
                    s, c = s[s >= 1], c[s >= 1]
                    b = (s - 1) // 16
                    assert np.all(ext[b, 0] <= c) and np.all(c <= ext[b, 1]), (k, v)
    # marginal reconstruction against the numpy up-down pass on the matrices the call built
    res = ctx.marginal_reconstruct(pr, level=0.95, alpha=0.7)
    _compare_marginal(res, MR.updown(pb, pr, MR.context_matrices(ctx, pb, K), 0.95), "order %d %s" % (order, model))
    ctx.close()


@pytest.mark.parametrize("order", [41, 300])
def test_root_max_and_reconstruction_under_death_rates(capi, order):
    pb = _problem(order)
    pr = _params(pb, "base")
    ref = MR.updown(pb, pr, _reference_matrices(pb, LAMBDAS, MUS, [1.0]), 0.95)
    ctx = capi.Context(pb)
    ctx.set_death_rates(MUS)
    got = ctx.root_max(LAMBDAS)
    want = np.array([fam[0].max() for fam in ref["root_inside"]])
    assert np.all(np.abs(got - want) <= SCORE_TOL * want) and np.all(want > 0)
    # cafe_reconstruct keeps no results to read back (cafe_get_matrix is CAFE_ERR_STATE after it), so the matrices are read
    # after cafe_root_max: the same rates through the same builder, hence the bits cafe_reconstruct works on
    mats = MR.context_matrices(ctx, pb, 1)[0]
    M, Rr = pb.max_family_size, pb.max_root_family_size
    root_prior = np.concatenate(([0.0], P.prior_uniform(Rr)))[:min(M, Rr) + 1].astype(np.float32)
    states = ctx.reconstruct(LAMBDAS, root_prior)
    for f in range(pb.n_families):
        assert np.array_equal(states[0, f], _pupko(pb, mats, root_prior, f)), f
    ctx.close()


def test_pvalues_per_family_and_validity_under_death_rates(capi):
    pb = _problem(41)
    pr = _params(pb, "base")
    ctx = capi.Context(pb)
    plain = ctx.pvalues(LAMBDAS, n_simulations=64, seed=7)
    ctx.set_death_rates(LAMBDAS)
    assert np.array_equal(ctx.pvalues(LAMBDAS, n_simulations=64, seed=7), plain)
    ctx.set_death_rates(MUS)
    pv = ctx.pvalues(LAMBDAS, n_simulations=64, seed=7)
    assert np.all(pv >= 0) and np.all(pv <= 1) and not np.array_equal(pv, plain)
    with pytest.raises(capi.CafeError, match="code 4"):                  # CAFE_ERR_STATE: the per-family kernel is lambda = mu
        ctx.score_per_family(pr, [0, 1], np.tile(LAMBDAS, (2, 1)))
    ctx.set_death_rates([0.007, -1e-9])                                  # an invalid mu is a value, as an invalid lambda is
    assert ctx.score(pr) == np.inf
    ctx.set_death_rates(None)
    assert np.all(np.isfinite(ctx.score_per_family(pr, [0, 1], np.tile(LAMBDAS, (2, 1)))))
    ctx.close()


# ------------------------------------------------------------------ bit identity with the lambda = mu path
@pytest.mark.parametrize("model", ["base", "gamma"])
def test_equal_death_rates_change_no_bit(capi, model):
    pb = _problem(300)
    pr = _params(pb, model)
    K = 1 if pr.multipliers is None else len(pr.multipliers)
    ctx = capi.Context(pb, max_categories=K)

    def call():
        v, fam = ctx.score(pr, alpha=0.7, per_family=True)
        return v, fam, [ctx.matrix(u, k) for k in range(K) for u in range(pb.n_nodes) if pb.parent[u] >= 0]

    def same(a, b):
        return (a[0] == b[0] and all(np.array_equal(a[1][key], b[1][key]) for key in a[1])
                and all(np.array_equal(x, y) for x, y in zip(a[2], b[2])))

    unset = call()
    assert np.isfinite(unset[0])
    ctx.set_death_rates(LAMBDAS)
    assert same(call(), unset)
    ctx.set_death_rates(MUS)
    assert call()[0] != unset[0]
    ctx.set_death_rates(None)
    assert same(call(), unset)
    ctx.close()


def test_graphs_are_not_replayed_across_a_change_of_mode(capi):
    pb = _problem(41)
    pr = _params(pb, "base")
    values = {}
    for graphs in (False, True):
        ctx = capi.Context(pb)
        ctx.set_graphs(graphs)
        seq = []
        for mus in (None, MUS, None, MUS):
            ctx.set_death_rates(mus)
            seq.append(ctx.score(pr))
        values[graphs] = seq
        ctx.close()
    assert values[True] == values[False]
    assert values[False][0] == values[False][2] and values[False][1] == values[False][3] and values[False][0] != values[False][1]
