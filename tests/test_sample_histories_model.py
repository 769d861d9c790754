"""tests/history_ref.py, the numpy statement of cafe_sample_histories, checked without a GPU: its frequencies against the
exact posteriors of tiny problems, and -- for every case the GPU replay uses -- that few histories are ambiguous on the
oracle's matrices and that the inputs tell five deliberately wrong samplers from the right one."""
import functools

import numpy as np
import pytest

import history_ref as HR
import marginal_ref as MR
from cafexp_amd import problem as P
from helpers import _explicit_problem
from oracle import oracle as O

N_DRAWS = 20000
LEFT_OUT = 1e-3


def _tiny(kind):
    rows = [dict(A=1, B=2, C=1), dict(A=0, B=3, C=2), dict(A=4, B=4, C=3), dict(A=0, B=0, C=1)]
    pb = _explicit_problem("((A:7.25,B:23.9):61.3,C:9.75);", rows, 4, 3 if kind == "base" else 4)
    # (0.005: the gamma case's largest multiplier must leave the longest branch below saturation, lambda t < 1)
    pr = P.Params(lambdas=np.array([0.005 if kind == "gamma" else 0.012]), prior=HR._prior(pb.max_root_family_size))
    if kind == "gamma":
        from cafexp_amd.gamma_rates import discrete_gamma
        pr.cat_probs, pr.multipliers = discrete_gamma(2, 0.7)
    if kind == "error_model":
        pb.n_deviations = 3
        pr.error_model = P.error_model_table(HR.THREE_TAPS, 4)
    assert pb.n_nodes <= 5 and pb.max_family_size <= 4
    return pb, pr


@pytest.mark.parametrize("kind", ["base", "gamma", "error_model"])
def test_frequencies_match_the_enumerated_posterior(oracle, kind):
    """Each frequency over 20 000 draws within 6 binomial standard errors of its exact probability: about 150 cells a case,
    a false alarm below 1e-6.  The exact p_increase / p_decrease are brute_force_family's; the exact size posteriors are
    updown_family's un-normalised ones, which must first reproduce brute_force_family's mean and p_increase to 1e-12."""
    pb, pr = _tiny(kind)
    mats = MR.oracle_matrices(pb, pr, oracle)
    got = HR.sample(pb, pr, mats, N_DRAWS, 12345)
    assert not got["failed"].any() and (got["sizes"] >= 0).all()
    root = MR.root_of(pb)
    n_cells = 0
    for f in range(pb.n_families):
        exact = MR.brute_force_family(pb, pr, mats, f, 0.95)
        ud = MR.updown_family(pb, pr, mats, f, 0.95, detail=True)
        for key in ("mean", "p_increase", "p_decrease"):
            ok = ~np.isnan(exact[key])
            assert np.allclose(ud[key][ok], exact[key][ok], rtol=1e-12, atol=1e-14), (kind, f, key)
        assert abs(got["log_evidence"][f] - exact["log_evidence"]) <= 1e-12 * abs(exact["log_evidence"]) + 1e-14
        x = got["sizes"][:, f, :]
        for v in range(pb.n_nodes):
            cells = [((x[:, v] == j).mean(), ud["post"][v][j] / ud["Z"]) for j in range(len(ud["post"][v]))]
            if v != root:
                p = int(pb.parent[v])
                cells += [((x[:, v] > x[:, p]).mean(), exact["p_increase"][v]), ((x[:, v] < x[:, p]).mean(), exact["p_decrease"][v])]
            for freq, prob in cells:
                se = np.sqrt(max(prob * (1 - prob), 0.0) / N_DRAWS)
                assert abs(freq - prob) <= 6 * se + 1e-12, (kind, f, v, freq, prob, se)
                n_cells += 1
        if kind == "gamma":                                  # the category: p_k Z_k / Z from brute_force_family's root vectors
            prior = np.asarray(pr.prior, dtype=np.float64)
            zk = np.array([pr.cat_probs[k] * (prior * exact["root_inside"][k]).sum() for k in range(2)])
            for k in range(2):
                freq, prob = (got["category"][:, f] == k).mean(), zk[k] / zk.sum()
                assert 0 < prob < 1 and abs(freq - prob) <= 6 * np.sqrt(prob * (1 - prob) / N_DRAWS), (f, k, freq, prob)
                n_cells += 1
    print("%s: %d cells within 6 standard errors" % (kind, n_cells))


# Where a mutant changes nothing by construction: at matrix order 2 the root's range 1..R is the single size 1, so no
# weighting of the root can draw anything else (asserted: the mutant's output is then identical).
NO_OP = {"order2": ("root_from_the_prior_alone", "prior_indexed_at_s")}


@functools.lru_cache(maxsize=None)
def _on_the_oracle(name):
    case = HR.CASES[name]()
    mats = HR.reference_matrices(case, O)
    return case, mats, HR.sample(case["pb"], case["pr"], mats, case["n_draws"], case["seed"])


@pytest.mark.parametrize("name", sorted(HR.CASES))
def test_replay_cases_are_sharp_and_tell_the_mutants_apart(oracle, name):
    case, mats, ref = _on_the_oracle(name)
    pb = case["pb"]
    share = ref["ambiguous"].mean()
    print("%s: %d of %d histories ambiguous (band %.3g)" % (name, ref["ambiguous"].sum(), ref["ambiguous"].size, HR.band(pb)))
    assert share <= LEFT_OUT                                 # if a seed breaks the cap, change the seed, not the cap
    assert not ref["failed"].any()
    for key, val in HR.recount(pb, ref["sizes"]).items():
        assert np.array_equal(val, ref[key])
    for mutant in HR.MUTANTS:
        mut = HR.sample(pb, case["pr"], mats, case["n_draws"], case["seed"], mutant=mutant)
        differ = ((mut["sizes"] != ref["sizes"]).any(axis=2) | (mut["category"] != ref["category"])).mean()
        print("%s: %s differs in %.1f %% of the histories" % (name, mutant, 100 * differ))
        if mutant in NO_OP.get(name, ()):
            assert pb.max_root_family_size == 1 and differ == 0
            continue
        assert differ > 0.01, (name, mutant, differ)


def test_cases_cover_what_they_claim():
    shape = {name: (c["pb"].matrix_size, len(set(HR.column_of(c["pb"]))), c["n_draws"]) for name, c in ((n, HR.CASES[n]()) for n in HR.CASES if n != "order751")}
    assert {2, 3, 64, 65, 129} <= {s[0] for s in shape.values()}
    assert {1, 255, 257} <= {s[1] for s in shape.values()} and {1, 64, 257} <= {s[2] for s in shape.values()}
    for name in ("order2", "order3", "order64", "order65", "order129"):
        assert HR.CASES[name]()["pb"].n_families == 300 and shape[name][2] == 65
    a, b = HR.CASES["root_below_M"]()["pb"], HR.CASES["root_above_M"]()["pb"]
    assert a.max_root_family_size < a.max_family_size and b.max_root_family_size > b.max_family_size
    taps = HR.CASES["three_taps"]()
    assert taps["pb"].counts.min() == 0 and taps["pb"].counts.max() == taps["pb"].max_family_size and taps["pr"].error_model.shape[1] == 3
    poly = HR.CASES["polytomy"]()["pb"]
    ch, root = MR.children_of(poly), MR.root_of(poly)
    assert len(ch[root]) == 4 and any(poly.leaf_taxon[c] >= 0 for c in ch[root])
    assert HR.CASES["caterpillar"]()["pb"].n_taxa == 8 and HR.CASES["gamma_k3"]()["K"] == 3
    assert len(set(HR.CASES["two_lambdas"]()["pb"].lambda_index)) == 2 and HR.CASES["death_rates"]()["mus"] is not None


def test_the_binding_exports_the_call():
    from cafexp_amd import capi
    assert "cafe_sample_histories" in capi.EXPORTS
    lib = capi.load()
    assert lib.cafe_sample_histories is not None and lib.cafe_abi_version() == 3
