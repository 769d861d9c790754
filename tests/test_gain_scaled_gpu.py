"""cafe_set_gain_scaling against tests/gain_scaled_ref.py (np.longdouble) below fp64's range, against the plain mode above it, and through
cafexp_hip.  lnl by test_lambda_per_family._close (1e-10, infinities exact), node outputs by test_gain_posterior_gpu._close (1e-10, floor 1e-290)."""
import subprocess
from contextlib import closing

import numpy as np
import pytest

import bd_lm_ref as R
import gain_posterior_ref as GP
import gain_ref as G
import gain_scaled_ref as S
from cafexp_amd import problem as P
from helpers import _explicit_problem
from test_gain_driver import DRIVER
from test_gain_gpu import _six_taxon
from test_gain_model import six_taxon_rates
from test_gain_posterior_gpu import _close, capi  # noqa: F401 (the fixture)
from test_gain_posterior_model import three_taxon
from test_lambda_per_family import _close as _close_lnl

wide = pytest.mark.skipif(not S.WIDE, reason="np.longdouble has fp64's exponent range here: no reference below 1e-308")
RATES = ((0.002, 0.0025, 0.003), tuple(G.RATES3[3]))


def tree32(M, Rr, star=False):
    """(problem, newick): balanced, 32 taxa, branches 3; families 0 / M, 15 with 1 at every third leaf (the last 20 beyond M = 16), ones; star: 40 leaves"""
    names = ["t%02d" % i for i in range(40 if star else 32)]
    level = [s + ":3" for s in names]
    while len(level) > 1 and not star:
        level = ["(%s,%s)%s" % (a, b, ":3" if len(level) > 2 else "") for a, b in zip(level[::2], level[1::2])]
    rows = [[M * (i % 2) for i in range(len(names))], [1 if i % 3 == 0 else 15 for i in range(31)] + [15 if M == 16 else 20], [1] * 32]
    newick = "(%s);" % ",".join(level) if star else level[0] + ";"
    return _explicit_problem(newick, [dict(zip(names, r)) for r in rows[:1 if star else 3]], M, Rr), newick


@pytest.mark.gpu
@pytest.mark.parametrize("case", [pytest.param(c, marks=wide) for c in ((16, 8), (64, 70), (129, 60), (16, 8, 1))] + [17, 129, "plain", "error", "missing"])
def test_scaled_against_the_longdouble_reference_and_the_plain_mode(capi, case):
    """(M, R, star): tree32 against the reference under both root rules, once the inputs bite by the reference alone (family 1: DESIGN section 8).
    The others: TREE3 (also with a zero column) and the six-taxon tree against the plain mode; NaN lambda; mode off again, bit for bit."""
    deep, star = isinstance(case, tuple), case == (16, 8, 1)
    if deep or isinstance(case, int):
        pb = tree32(*case)[0] if deep else three_taxon(case)
        pr = P.Params(lambdas=np.ones(1), prior=P.prior_uniform(pb.max_root_family_size))
        runs = [(*r, a) for r in RATES[:1 if star else 2] for a in (0.0, 0.2)] if deep else [(*G.RATES3[1], 0.2), (*G.RATES3[1, :2], 0.0, 1.0)]
    else:
        pb = _six_taxon(41, case == "error", case == "missing")
        pr, runs = R.params(pb, "error" if case == "error" else "base"), [(*(x[0] for x in six_taxon_rates(pb)), 0.2)]
    fam = [0] if star else list(range(pb.n_families)) + [capi.CAFE_FAMILY_ABSENT]   # (the star's absent profile: DESIGN section 8)
    with closing(capi.Context(pb)) as ctx:
        for *rates, absent in runs:
            args = (pr, fam, *map(np.atleast_1d, rates), absent)
            plain, scaled, again = [(ctx.set_gain_scaling(on), ctx.gain_posterior_dense(*args, want_posterior=True))[1] for on in (False, True, False)]
            assert all(np.array_equal(plain[key], again[key], equal_nan=True) for key in plain)
            want = S.table(pb, fam, rates, pr.prior, absent) if deep else plain
            if deep:                               # the inputs bite, by the reference alone: top[i] is family i's largest root likelihood
                top = want["top"]
                assert top[0] < S.LD("1e-400") and plain["lnl"][0] == -np.inf and (star or (top[1] < S.LD(2.2250738585072014e-308) and top[2] > 1e-10))
                assert star or tuple(rates) != RATES[0] or top[1] >= S.LD(5e-324)          # under RATES[0] inside the denormal range
            else:
                assert np.isfinite(plain["lnl"]).all() == (absent < 1) and not np.isnan(scaled["lnl"]).any() and np.isfinite(plain["lnl"]).any()
            _close_lnl(scaled["lnl"], want["lnl"])
            for key in GP.KEYS:
                _close(scaled[key], want[key], key)
            ctx.set_gain_scaling(True)
            for rule, key in (("max", "lnl_max"), ("sum", "lnl"))[0 if deep else 1:]:
                ctx.set_root_rule(rule)
                _close_lnl(ctx.score_gain(*args), want[key])
        if case == "plain":
            nan = (pr, fam, [np.nan, R.LAMBDAS[1]], R.MUS, [0.003, 0.001], 0.1)
            assert np.isnan(ctx.score_gain(*nan)).all() and np.isnan(ctx.gain_posterior_dense(*nan)["lnl"]).all()


@pytest.mark.gpu
def test_place_and_batch_change_no_bit(capi, monkeypatch):
    pb, pr, rates = tree32(16, 8)[0], P.Params(lambdas=np.ones(1), prior=P.prior_uniform(8)), [[r] for r in RATES[0]]
    pool, alone = np.array([0, 1, 2, capi.CAFE_FAMILY_ABSENT]), None
    for n, batch in ((1, "0"), (128, "0"), (129, "0"), (257, "0"), (257, "1")):      # "0": as many entries a batch as fit
        monkeypatch.setenv("CAFE_PER_FAMILY_BATCH", batch)
        with closing(capi.Context(pb)) as ctx:
            ctx.set_gain_scaling(True)
            alone = alone or [ctx.gain_posterior_dense(pr, [f], *rates, 0.2) for f in pool]
            got = ctx.gain_posterior_dense(pr, pool[np.arange(n) % 4], *rates, 0.2)
        for key in ("lnl", "p_gain"):
            assert np.array_equal(got[key], [alone[i % 4][key][0] for i in range(n)], equal_nan=True), (key, n, batch)


@wide
@pytest.mark.gpu
def test_driver_prints_a_finite_objective_where_the_plain_prune_answers_inf(tmp_path):
    """--gain NU --gain-dense at fixed rates: -lnL inf; with --gain-scaled the reference's objective at 1e-10; alone, refused"""
    pb, newick = tree32(16, 8)
    (tmp_path / "tree.txt").write_text(newick + "\n")
    (tmp_path / "families.txt").write_text("Desc\tFamily ID\t" + "\t".join(pb.taxa) + "\n" +
                                           "".join("(null)\tf%d\t%s\n" % (i, "\t".join(map(str, row))) for i, row in enumerate(pb.counts)))
    cmd = [DRIVER, "-t", str(tmp_path / "tree.txt"), "-i", str(tmp_path / "families.txt"), "--gain", str(RATES[0][2]), "-l", str(RATES[0][0]),
           "--mu", str(RATES[0][1]), "--root-absent", "0.2", "--sizes", "16,8", "-o", str(tmp_path / "out")]
    refused, plain, scaled = [subprocess.run(cmd + more, capture_output=True, text=True, timeout=300)
                              for more in (["--gain-scaled"], ["--gain-dense"], ["--gain-dense", "--gain-scaled"])]
    assert refused.returncode == 1 and "--gain-scaled is the scaled mode of the dense prune: give --gain-dense with it" in refused.stderr
    assert plain.returncode == 0 and '"gain_dense_mode": "plain", "neg_lnl": inf' in plain.stdout, plain.stderr
    assert scaled.returncode == 0 and '"gain_dense_mode": "scaled", "neg_lnl": ' in scaled.stdout, scaled.stderr
    lnl = S.table(pb, [0, 1, 2, -1], RATES[0], P.prior_uniform(8), 0.2)["lnl"]
    _close_lnl([float(scaled.stdout.split('"neg_lnl": ')[1].split(",")[0])], [-lnl[:3].sum() + 3 * np.log(-np.expm1(lnl[3]))])
