"""cafe_gain_score_gradient (gain_gradient_kernel.h) against the complex-step reference of tests/gain_gradient_ref.py on the cases of
tests/gain_marginal_ref.py -- M + 1 = 63 / 64 / 65 / 80 / 129, R on either side, a polytomy, an error model -- and one case with two
rate indices on the "three" tree.  Every output: |got - ref| <= 1e-12 + 1e-10 c |ref| (gradient_ref.close's form, the bound of
tests/test_gradient_gpu.py), c the entry's own cancellation factor over the branches, 1 for a single branch's score; c < 1e3 is
asserted on the reference alone.  Worst measured on the MI355X: DESIGN section 8.  d_lambda, d_mu, d_nu also against central
differences of cafe_score_gain, step 1000 quanta, to 1e-6 (test_gradient_gpu.py's)."""
import functools
from contextlib import closing

import numpy as np
import pytest

import gain_gradient_ref as GG
import gain_marginal_ref as GM
from test_gain_posterior_gpu import capi  # noqa: F401 (the fixture)

C_BOUND = 1000.0
TWO = (64, 40, "three", False, 2)                      # two rate indices: the second on C (a leaf), D (under the root) and (E,F) (interior)
CASES = [c + (1,) for c in GM.CASES] + [TWO]
RATES2 = ([0.0051, 0.0031], [0.00408, 0.0036], [0.00102, 0.0021])
KEYS = GG.RATE_KEYS + GG.BRANCH_KEYS


def _problem(M, Rr, tree, error, n_lambdas):
    pb, pr = GM.problem(M, Rr, tree, error)
    if n_lambdas == 2:
        names = sorted(c for c in GM.TREES[tree] if c.isalpha())
        leaf = {names[pb.leaf_taxon[v]]: v for v in range(pb.n_nodes) if pb.leaf_taxon[v] >= 0}
        pb.lambda_index[[leaf["C"], leaf["D"], int(pb.parent[leaf["E"]])]], pb.n_lambdas, pb.single_lambda = 1, 2, False
        pr.lambdas = np.ones(2)
    return pb, pr, RATES2 if n_lambdas == 2 else tuple([r] for r in GM.RATES), np.array(list(range(pb.n_families)) + [-1])


@functools.lru_cache(maxsize=None)
def _reference(case):
    pb, pr, rates, pool = _problem(*case)
    return GG.table(pb, pool, *rates, pr.prior, GM.ABSENT, pr.error_model)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_the_reference_reports_the_cancellation_the_bound_assumes(case):
    worst = max(float(np.nanmax(_reference(case)["cancel_" + k])) for k in GG.RATE_KEYS)
    print("largest cancellation factor %.1f" % worst)
    assert worst < C_BOUND


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=str)
def test_every_tile_edge_and_tree_shape_against_the_complex_step_reference(capi, case):
    """Lists of 1, 128 and 129 entries (a repeated index and CAFE_FAMILY_ABSENT among them); the small workspace_limit cuts the 129 into
    two batches (tests/test_gain_marginal_gpu.py)"""
    pb, pr, rates, pool = _problem(*case)
    want, small, got = _reference(case), 6 * pb.matrix_size * 128 * 8, {}
    for n, limit in ((1, 0), (128, 0), (129, 0), (129, small)):
        at, worst = (np.arange(n) + 3) % len(pool), 0.0
        with closing(capi.Context(pb, workspace_limit=limit)) as ctx:
            ctx.set_gain_scaling(True)                  # not read by this call
            got[n, limit] = res = ctx.gain_score_gradient(pr, pool[at], *rates, GM.ABSENT)
            ctx.set_gain_scaling(False)
            ctx.set_root_rule("sum")
            assert np.array_equal(res["lnl"], ctx.score_gain(pr, pool[at], *rates, GM.ABSENT))
        for key in KEYS:
            g, r = res[key], want[key][at]
            assert np.array_equal(np.isnan(g), np.isnan(r)), (n, limit, key)
            factor = np.minimum(C_BOUND, np.maximum(1.0, want["cancel_" + key][at])) if key in GG.RATE_KEYS else 1.0
            with np.errstate(invalid="ignore"):
                worst = max(worst, float(np.nanmax(np.abs(g - r) / (1e-12 + 1e-10 * factor * np.abs(r)))))
        print("n %d limit %d: worst |got - ref| / bound %.3g" % (n, limit, worst))
        assert worst <= 1.0, (n, limit, worst)
    for key in ("lnl",) + KEYS:                         # place and batch cut change no bit
        for (n, limit), res in got.items():
            same = np.nonzero((np.arange(n) + 3) % len(pool) == 3 % len(pool))[0]
            assert all(np.array_equal(res[key][i], got[1, 0][key][0], equal_nan=True) for i in same), (key, n, limit)
        assert np.array_equal(got[129, 0][key], got[129, small][key], equal_nan=True), key


@pytest.mark.gpu
@pytest.mark.parametrize("case", [GM.CASES[1] + (1,), TWO], ids=str)
def test_central_differences_of_score_gain(capi, case):
    pb, pr, rates, pool = _problem(*case)
    with closing(capi.Context(pb)) as ctx:
        ctx.set_root_rule("sum")
        got = ctx.gain_score_gradient(pr, pool, *rates, GM.ABSENT)
        for which, q in [(w, q) for w in range(3) for q in range(pb.n_lambdas)]:
            vals = []
            for sign in (-1, 1):
                moved = [np.array(r, dtype=float) for r in rates]
                moved[which][q] = (int(moved[which][q] * 1e9) + sign * 1000 + 0.5) / 1e9            # (+ 0.5 quantum: the truncation lands on the grid point)
                vals.append(ctx.score_gain(pr, pool, *moved, GM.ABSENT))
            fd, g = (vals[1] - vals[0]) / 2e-6, got[GG.RATE_KEYS[which]][:, q]
            err, bound = np.abs(fd - g), 1e-6 * np.abs(g) + 4 * np.finfo(float).eps * np.abs(vals[0]) / 2e-6
            print("%s[%d]: worst |fd - g| / bound %.3g" % (GG.RATE_KEYS[which], q, (err / bound).max()))
            assert np.all(err <= bound), (which, q)


@pytest.mark.gpu
def test_identities_and_edge_cases(capi):
    pb, pr, rates, pool = _problem(*TWO)
    lam, mu, nu = (np.array(r) for r in rates)
    root, second = int(np.where(pb.parent < 0)[0][0]), np.nonzero(pb.lambda_index == 1)[0]
    with closing(capi.Context(pb)) as ctx:
        pr.lambdas = lam                               # nu = 0 and root_absent = 0: the base model's own score vectors under the sum rule
        ctx.set_death_rates(mu)
        base, got = ctx.score_gradient(pr, "sum"), ctx.gain_score_gradient(pr, pool[:-1], lam, mu, np.zeros(2), 0.0)
        ref0 = GG.table(pb, pool[:-1], lam, mu, np.zeros(2), pr.prior, 0.0)                  # for each entry's own cancellation factor
        for key in ("d_lambda", "d_mu"):
            factor = np.minimum(C_BOUND, np.maximum(1.0, ref0["cancel_" + key]))
            assert np.all(np.abs(got[key] - base[key]) <= 1e-12 + 1e-10 * factor * np.abs(base[key])), key
        assert np.isnan(got["d_alpha"][:, root]).all() and np.isfinite(got["d_nu"]).all()
        # a saturated key (lambda t >= 1 at lambda = mu, every branch of the second index) adds exactly 0
        sat = ctx.gain_score_gradient(pr, pool, [lam[0], 0.5], [mu[0], 0.5], nu, GM.ABSENT)
        ok = np.isfinite(sat["lnl"])
        assert ok.sum() >= 2 and np.isfinite(sat["d_lambda"][ok][:, 0]).all() and all(np.isnan(sat[k][~ok]).all() for k in KEYS)
        assert all(np.all(sat[k][ok][:, 1] == 0.0) for k in GG.RATE_KEYS) and all(np.all(sat[k][ok][:, second] == 0.0) for k in GG.BRANCH_KEYS)
        # lambda_q = 0: the Poisson limit, NaN in that index's three scores
        poi = ctx.gain_score_gradient(pr, pool, [lam[0], 0.0], mu, nu, GM.ABSENT)
        assert np.isfinite(poi["lnl"]).all() and all(np.isnan(poi[k][:, 1]).all() and np.isfinite(poi[k][:, 0]).all() for k in GG.RATE_KEYS)
    pb.counts[0, 0], pb.missing_counts = capi.CAFE_COUNT_MISSING, True          # a missing leaf's branch adds exactly 0
    leaf = int(np.nonzero(pb.leaf_taxon == 0)[0][0])
    with closing(capi.Context(pb)) as ctx:
        mis = ctx.gain_score_gradient(pr, [0, 1], lam, mu, nu, GM.ABSENT)
    assert all(mis[k][0, leaf] == 0.0 and mis[k][1, leaf] != 0.0 for k in GG.BRANCH_KEYS) and np.isfinite(mis["d_lambda"]).all()
