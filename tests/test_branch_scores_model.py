"""The model behind cafe_branch_scores and the rate-shift scan, on the CPU (tests/branch_scores_ref.py).

  * the two statements of the per-branch log-rate score -- a complex-step prune with the step on one branch's rates, and the
    reverse-mode contraction kept per branch -- agree under gradient_ref's cancellation-factor bound;
  * the sum identities: over the branches of lambda index q, rate (birth) adds up to lambda_q d_lambda_q and death to
    mu_q d_mu_q; over all branches rate adds up to sum_k m_k d_multiplier_k -- to that bound;
  * three deliberately wrong references (the slot taken from the lambda index instead of the node; the mu term dropped; the
    category coefficient m_k dropped) are each told from the right one by more than 100 x the bound on the GPU tests' inputs;
  * a planted shift: 300 families simulated on an 8-taxon tree (M = 40) with the clade (E, F) at 4 x the rate; lambda fitted
    on the reference lnL; the planted clade has the smallest clade p and its Holm-adjusted p is below 1e-3; on a null
    simulation from the same generator no Holm-adjusted p is below 0.05.  (Seeds 1 and 101: picked so that the reference
    satisfies this.)
  * the new names are exported, the ABI version is 3, and the driver refuses what does not combine with --rate-shift-scan."""
import os
import subprocess

import numpy as np
import pytest

import branch_scores_ref as BR
import gradient_ref as GR
import test_gradient_shapes as TS
from helpers import DATA
from test_branch_scores_shapes import C_BOUND, column_case, pair_case

TWO_WAYS = [(15, 12), (16, 40), (64, 40)]
HERE = os.path.dirname(os.path.abspath(__file__))
DRIVER = os.path.join(os.path.dirname(HERE), "cafexp_amd", "host", "cafexp_hip")


@pytest.mark.parametrize("config", sorted(TS.CONFIGS))
@pytest.mark.parametrize("M,R", TWO_WAYS)
def test_the_two_statements_agree(M, R, config):
    for rule in ("max", "sum"):
        pb, pr, mus, ref = pair_case(M, R, config, rule)
        cs = BR.complex_step(pb, pr, mus, rule)
        assert np.array_equal(cs["failed"], ref["failed"])
        GR.close(BR.as_gradient(cs), BR.as_gradient(ref), C_BOUND, "complex step against reverse: M %d R %d %s %s" % (M, R, config, rule))
        assert np.all(np.abs(cs["family_lnl"] - ref["family_lnl"]) <= 1e-12 + 1e-10 * np.abs(ref["family_lnl"]))


def _within(got, want, factor):
    return np.all(np.abs(got - want) <= 1e-12 + 1e-10 * np.minimum(C_BOUND, np.maximum(1.0, factor)) * np.abs(want))


@pytest.mark.parametrize("config", sorted(TS.CONFIGS))
@pytest.mark.parametrize("M,R", TS.PAIRS)
def test_the_sum_identities(M, R, config):
    for rule in ("max", "sum"):
        pb, pr, mus, ref = pair_case(M, R, config, rule)
        lam, mu = BR._rates(pb, pr, mus)
        nonroot = pb.parent >= 0
        for q in range(pb.n_lambdas):
            sel = nonroot & (pb.lambda_index == q)
            first = "rate" if mus is None else "birth"
            assert _within(ref[first][:, sel].sum(axis=1), lam[q] * ref["d_lambda"][:, q], ref["cancel_d_lambda"][:, q]), (rule, q)
            if mus is not None:
                assert _within(ref["death"][:, sel].sum(axis=1), mu[q] * ref["d_mu"][:, q], ref["cancel_d_mu"][:, q]), (rule, q)
        if pr.multipliers is not None:
            m = np.asarray(pr.multipliers)
            want = ref["d_multiplier"] @ m
            room = (ref["cancel_d_multiplier"] * np.abs(ref["d_multiplier"])) @ np.abs(m)      # the sum of |terms| behind the sum
            assert np.all(np.abs(ref["rate"][:, nonroot].sum(axis=1) - want) <= 1e-12 + 1e-10 * np.minimum(C_BOUND * np.abs(want), room)), rule


def _told_apart(mut, ref):
    big = False
    for key in BR.NAMES:
        if key in ref:
            ok = ~np.isnan(ref[key])
            big = big or bool(np.max(np.abs(mut[key][ok] - ref[key][ok]) / (1e-12 + 1e-10 * C_BOUND * np.abs(ref[key][ok]))) > 100)
    return big


@pytest.mark.parametrize("M,R", TS.PAIRS)
def test_the_inputs_tell_a_wrong_reference_from_the_right_one(M, R):
    for config in sorted(TS.CONFIGS):
        for rule in ("max", "sum"):
            pb, pr, mus, ref = pair_case(M, R, config, rule)
            for name in BR.MUTANTS:
                mut = BR.reverse(pb, pr, mus, rule, mutant=name)
                label = "%s M %d R %d %s %s" % (name, M, R, config, rule)
                if name == "multiplier_dropped" and pr.multipliers is None:
                    for key in BR.NAMES:                     # the base model has no coefficient to drop
                        assert key not in ref or np.array_equal(mut[key], ref[key], equal_nan=True), label
                    continue
                assert _told_apart(mut, ref), label
                with pytest.raises(AssertionError):
                    GR.close(BR.as_gradient(mut), BR.as_gradient(ref), C_BOUND, label)


def test_the_column_cases_tell_the_mutants_apart_too():
    pb, pr, mus, ref = column_case(129)
    for name in BR.MUTANTS:
        assert _told_apart(BR.reverse(pb, pr, mus, "max", mutant=name), ref), name


# ------------------------------------------------------------------------------------------------------ the statistic
def test_holm_is_the_step_down_adjustment():
    p = np.array([0.01, np.nan, 0.04, 0.03, 0.5])
    assert np.allclose(BR.holm(p), [0.04, np.nan, 0.09, 0.09, 0.5], equal_nan=True)
    assert np.isnan(BR.holm([np.nan, np.nan])).all()


def test_a_direction_inside_the_searched_parameters_is_not_testable():
    rng = np.random.default_rng(5)
    z = rng.standard_normal((200, 5))
    z[:, 4] = z[:, 0] + z[:, 1]                              # the global score is the sum of two branch scores
    total, gram = z.sum(axis=0), z.T @ z
    T = np.eye(5)[:, 4:]
    both = BR.score_test(total, gram, np.array([1.0, 1, 0, 0, 0]), T)
    one = BR.score_test(total, gram, np.array([1.0, 0, 0, 0, 0]), T)
    assert not both["testable"] and np.isnan(both["p"]) and one["testable"] and 0 < one["p"] <= 1
    free = BR.score_test(total, gram, np.array([0, 0, 1.0, 0, 0]), np.zeros((5, 0)))
    assert np.isclose(free["stat"], total[2] ** 2 / gram[2, 2]) and np.isclose(free["multiplier"], np.exp(total[2] / gram[2, 2]))


def test_a_planted_shift_is_found_and_a_null_table_is_clean():
    res = BR.planted_scan(BR.planted_counts(1, 4.0))
    top, below = BR.planted_nodes(res["pb"])
    assert len(below) == 3 and res["pb"].n_taxa == 8 and res["pb"].max_family_size <= 40 and res["pb"].n_families == 300
    i = res["nodes"].index(top)
    print("planted: lambda %.5f, clade statistic %.2f, p %.3g, Holm %.3g, one-step multiplier %.2f"
          % (res["lam"], res["clade"][i]["stat"], res["clade"][i]["p"], res["clade_holm"][i], res["clade"][i]["multiplier"]))
    assert abs(res["total"][-1]) <= 1e-2                      # the fit: the total lambda score is zero
    assert int(np.nanargmin([t["p"] for t in res["clade"]])) == i
    assert res["clade_holm"][i] < 1e-3 and res["clade"][i]["multiplier"] > 1
    null = BR.planted_scan(BR.planted_counts(101, 1.0))
    print("null: lambda %.5f, smallest Holm p: branch %.3g, clade %.3g" % (null["lam"], np.nanmin(null["branch_holm"]), np.nanmin(null["clade_holm"])))
    assert not np.any(null["branch_holm"] < 0.05) and not np.any(null["clade_holm"] < 0.05)


# ------------------------------------------------------------------------------------------------- exports and refusals
def test_the_new_entries_are_exported_and_the_abi_version_stays():
    from cafexp_amd import capi
    lib = capi.load()
    for name in ("cafe_branch_scores", "cafe_branch_scores_dim", "cafe_weighted_gram"):
        assert name in capi.EXPORTS and getattr(lib, name) is not None
    assert lib.cafe_abi_version() == 3
    for name in ("branch_scores", "branch_scores_dim"):
        assert callable(getattr(capi.Context, name))
    assert callable(capi.weighted_gram)


def test_the_driver_refuses_what_does_not_combine(tmp_path):
    assert os.path.exists(DRIVER), "cafexp_hip missing: run __graft_entry__.build()"
    common = ["-t", os.path.join(DATA, "synth20_tree.txt"), "-i", os.path.join(DATA, "synth20_families.txt"), "--rate-shift-scan", "-o", str(tmp_path / "out")]
    for extra, message in ((["-b"], "-b is not supported with it"), (["--gpus", "2"], "--gpus is not supported with it"),
                           (["--simulate", "10", "-l", "0.01"], "--simulate is not supported with it")):
        r = subprocess.run([DRIVER] + common + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--rate-shift-scan" in r.stderr and message in r.stderr, (extra, r.stderr)
    assert not os.path.exists(str(tmp_path / "out"))
