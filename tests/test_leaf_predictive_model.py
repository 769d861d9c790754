"""What cafe_leaf_predictive is defined to compute, on the CPU: the entry is exported, the two statements of
tests/leaf_predictive_ref.py agree, the observed count carries the evidence, a leaf's own count reaches its row only through
the three probabilities, and the inputs of the GPU tests (tests/test_leaf_predictive_shapes.py) are fit for their purpose: no
cell fails, no total underflows, the cancellation in sd stays below the constant the GPU tests put into their bound, and each
of the reference's five deliberately wrong statements is told from the right one by more than 100 x that bound.

The GPU tests hold every sd to min(C_BOUND, its own 1 + (mean - x)^2 / var) with C_BOUND = 100 and everything else to 1.  Measured here
(C_MEASURED, printed by test_the_cancellation_stays_below_the_constant_of_the_gpu_tests): the largest factor over all input sets is
99.3; that test's docstring has the figures of the inputs and rates that were not taken."""
import dataclasses
import os
import re

import numpy as np
import pytest

import leaf_predictive_ref as LR
from cafexp_amd import capi
from test_gradient_shapes import CONFIGS, PAIRS
from test_leaf_predictive_shapes import C_BOUND, _pair_case, input_sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_MEASURED = 99.3


def test_the_entry_is_exported_and_the_abi_version_stays():
    header = open(os.path.join(ROOT, "include", "cafe_mi355x.h")).read()
    assert re.search(r"^int cafe_leaf_predictive\(cafe_ctx\* ctx, const cafe_params\* params, const cafe_leaf_predictive_out\* out\);", header, re.M)
    assert re.search(r"^#define CAFE_ABI_VERSION 3$", header, re.M)
    assert "cafe_leaf_predictive" in capi.EXPORTS
    fields = re.search(r"typedef struct cafe_leaf_predictive_out \{(.*?)\}", header, re.S).group(1)
    assert re.findall(r"\*\s*(\w+);", fields) == [name for name, _ in capi.CafeLeafPredictiveOut._fields_]
    assert hasattr(capi.Context, "leaf_predictive")


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("M,R", PAIRS[::3])
def test_the_two_routes_agree(M, R, config):
    pb, pr, mus, ref = _pair_case(M, R, config)
    brute = LR.reference(pb, pr, LR.matrices(pb, pr, mus), route="brute")
    LR.close(brute, ref, C_BOUND, "brute force against up/down M %d R %d %s" % (M, R, config))
    assert np.all(np.abs(brute["W"] - ref["W"]) <= 1e-10 * ref["W"])


def test_the_observed_count_carries_the_evidence():
    for label, (pb, pr, mus, ref) in input_sets():
        Z = np.repeat(ref["Z"][:, None], ref["w_obs"].shape[1], axis=1)
        assert np.all(np.abs(ref["w_obs"] - Z) <= 1e-10 * Z), label


def test_a_leafs_own_count_reaches_its_row_only_through_x():
    """another count at one leaf: w of that leaf is what it was, so mean, sd and W are, and the three probabilities are those of
    the old w at the new x; the other leaves' rows move"""
    pb, pr, mus, ref = _pair_case(16, 14, "gamma_err_rho_0.25")
    mats = LR.matrices(pb, pr, mus)
    t = 2
    other = dataclasses.replace(pb, counts=pb.counts.copy())
    other.counts[:, t] = (pb.counts[:, t] + 3) % (pb.max_family_size + 1)
    new = LR.reference(other, pr, mats)
    for key in ("mean", "sd", "W"):
        assert np.all(np.abs(new[key][:, t] - ref[key][:, t]) <= 1e-13 * np.abs(ref[key][:, t])), key
    assert np.any(new["p_obs"][:, t] != ref["p_obs"][:, t])
    assert np.any(np.delete(new["mean"], t, axis=1) != np.delete(ref["mean"], t, axis=1))
    for f in range(pb.n_families):                          # p_obs at the new x is the brute-force Z(x) / W of the old table
        swapped = dataclasses.replace(pb, counts=pb.counts.copy())
        swapped.counts[f, t] = other.counts[f, t]
        z = LR.reference(swapped, pr, mats)["Z"][f]
        assert abs(new["p_obs"][f, t] - z / ref["W"][f, t]) <= 1e-10 * new["p_obs"][f, t] + 1e-300


def test_no_cell_fails_and_no_total_underflows():
    for label, (pb, pr, mus, ref) in input_sets():
        assert not ref["failed"].any(), label
        for key in LR.KEYS:
            assert not np.isnan(ref[key]).any(), (label, key)
        assert ref["W"].min() > 1e-250, (label, ref["W"].min())
        assert np.all(np.abs(ref["p_below"] + ref["p_obs"] + ref["p_above"] - 1) <= 1e-12), label


def test_the_figure_in_this_file_is_the_one_measured():
    worst = max(LR.worst_cancellation(case[3]) for _, case in input_sets())
    assert abs(worst - C_MEASURED) <= 0.05 * C_MEASURED


def test_the_cancellation_stays_below_the_constant_of_the_gpu_tests():
    """The largest 1 + (mean - x)^2 / var is 99.3 (300 distinct families, gamma: family 103, species B observed at 12, mean 0.97,
    sd 1.11); the pairs reach 58.5 (base), 40.5 (base, error model, rho 4) and 19.2 (gamma), the table of taps at 0 and M 9.5.
    With test_gradient_shapes' random rows as drawn, every species from 0..12 on its own, the pairs reached 487.0 (M 64, R 40, base:
    species J at 12 with every relative at 0 or 1 -- mean 0.28, sd 0.53) and 21 of the 30 exceeded 100.  Rates did not tame
    that: with the lambdas and death rates of every configuration multiplied by 2, 3, 5 and 6.5 the largest factor was 332, 316,
    281 and 253, and at 7.2 the longest branch reaches lambda t = 1, where its key is marked zero.  So the pairs' counts were
    tamed (_tamed of test_leaf_predictive_shapes) and the bound stayed."""
    worst = {label: LR.worst_cancellation(case[3]) for label, case in input_sets()}
    top = max(worst, key=worst.get)
    print("largest 1 + (mean - x)^2 / var: %.1f (%s); %d of %d input sets above 100" % (worst[top], top, sum(v > 100 for v in worst.values()), len(worst)))
    assert worst[top] <= C_BOUND <= 100


def _ratio(mut, ref):
    worst = 0.0
    for key in LR.KEYS:
        ok = ~np.isnan(ref[key])
        if np.isnan(mut[key][ok]).any():
            return np.inf
        worst = max(worst, float(np.max(np.abs(mut[key][ok] - ref[key][ok]) / (1e-12 + 1e-10 * C_BOUND * np.abs(ref[key][ok])))))
    return worst


def test_the_inputs_tell_a_wrong_statement_from_the_right_one():
    for label, (pb, pr, mus, ref) in input_sets():
        mats = LR.matrices(pb, pr, mus)
        for name in LR.MUTANTS:
            mut = LR.reference(pb, pr, mats, mutant=name)
            if (name == "err_indexed_at_c" and pr.error_model is None) or (name == "mixed_after_normalising" and pr.multipliers is None):
                LR.close(mut, ref, C_BOUND, name)            # no error model to misread, one category to mix: the right statement
                continue
            ratio = _ratio(mut, ref)
            assert ratio > 100, (label, name, ratio)
            with pytest.raises(AssertionError):
                LR.close(mut, ref, C_BOUND, name)
