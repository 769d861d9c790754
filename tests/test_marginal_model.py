"""The marginal reconstruction's model, on the CPU: the numpy up-down pass of tests/marginal_ref.py against a brute-force
enumeration of every interior assignment, on trees of 3-5 leaves with M <= 10 -- every output to 1e-13 relative -- and its
root inside vector against the oracle's prune.  Matrices come from oracle.build_matrix.  Also: the library exports the entry
point and the driver names its flag."""
import os
import subprocess

import numpy as np
import pytest

import marginal_ref as MR
from cafexp_amd import problem as P
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-13


def _problem(newick, rows, M, R, lambda_tree=None, n_dev=0):
    tree = P.parse_newick(newick)
    species = sorted(rows[0])
    table = np.array([[r[s] for s in species] for r in rows], dtype=np.int32)
    lt = P.parse_newick(lambda_tree, lambda_tree=True) if lambda_tree else None
    return P.build_problem(tree, species, ["f%d" % i for i in range(len(rows))], table, lambda_tree=lt, root_filter=False,
                           max_family_size=M, max_root_family_size=R, n_deviations=n_dev)


def _cases():
    out = {}
    # a binary tree of five leaves
    pb = _problem("((A:1,B:2):3,((C:1,D:1):2,E:4):1);", [dict(A=1, B=2, C=3, D=1, E=2), dict(A=0, B=1, C=0, D=0, E=5), dict(A=4, B=4, C=4, D=4, E=4)], 8, 6)
    out["binary5"] = (pb, P.Params(lambdas=np.array([0.05]), prior=P.prior_uniform(6)))
    # a polytomy at the root and one below it
    pb = _problem("((A:2,B:2,C:1):3,D:5,E:4);", [dict(A=1, B=2, C=3, D=1, E=2), dict(A=0, B=0, C=2, D=1, E=0)], 7, 7)
    out["polytomy"] = (pb, P.Params(lambdas=np.array([0.03]), prior=P.prior_uniform(7)))
    # two lambdas with a lambda tree
    pb = _problem("((A:1,B:2):3,(C:1,D:1):2);", [dict(A=1, B=2, C=3, D=1), dict(A=5, B=0, C=1, D=2)], 9, 5,
                  lambda_tree="((A:1,B:1):1,(C:2,D:2):2);")
    out["two_lambdas"] = (pb, P.Params(lambdas=np.array([0.02, 0.11]), prior=P.prior_uniform(5)))
    # a 3-tap error model
    pb = _problem("((A:1,B:2):3,C:4);", [dict(A=1, B=2, C=3), dict(A=0, B=1, C=0), dict(A=6, B=5, C=6)], 6, 5, n_dev=3)
    pr = P.Params(lambdas=np.array([0.06]), prior=P.prior_uniform(5))
    pr.error_model = P.error_model_table(P.default_error_model(6), 6)
    out["error_model"] = (pb, pr)
    # a Poisson prior
    pb = _problem("((A:1,B:2):3,(C:1,D:1):2);", [dict(A=1, B=2, C=3, D=1), dict(A=2, B=2, C=0, D=7)], 10, 8)
    out["poisson"] = (pb, P.Params(lambdas=np.array([0.04]), prior=P.prior_poisson(8, 2.5)))
    # the gamma model, two categories
    pb = _problem("((A:1,B:2):3,C:4);", [dict(A=1, B=2, C=3), dict(A=3, B=0, C=1)], 8, 6)
    pr = P.Params(lambdas=np.array([0.05]), prior=P.prior_uniform(6))
    pr.cat_probs, pr.multipliers = O.discrete_gamma(2, 0.7)
    out["gamma2"] = (pb, pr)
    return out


CASES = _cases()


def _close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(a)
    assert np.all(np.abs(a[ok] - b[ok]) <= TOL * np.abs(b[ok])), (a, b)


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("level", [0.95, 0.5])
def test_updown_equals_brute_force(name, level):
    pb, pr = CASES[name]
    mats = MR.oracle_matrices(pb, pr, O)
    for f in range(pb.n_families):
        ud = MR.updown_family(pb, pr, mats, f, level)
        bf = MR.brute_force_family(pb, pr, mats, f, level)
        assert ud["failed"] == bf["failed"] == 0
        for key in ("mean", "p_increase", "p_decrease"):
            _close(ud[key], bf[key])
        _close(ud["log_evidence"], bf["log_evidence"])
        for k in range(len(mats)):
            _close(ud["root_inside"][k], bf["root_inside"][k])
        for key in ("mode", "lo", "hi"):
            # integers are exact unless the enumeration itself sits on a tie
            tie = bf[key + "_gap"] <= 1e-12
            assert np.array_equal(ud[key][~tie], bf[key][~tie]), (key, ud[key], bf[key])
        assert np.all(ud["lo"] <= ud["mode"]) and np.all(ud["mode"] <= ud["hi"])
        s = ud["p_increase"] + ud["p_decrease"]
        assert np.all((s[~np.isnan(s)] >= 0) & (s[~np.isnan(s)] <= 1 + 1e-12))


@pytest.mark.parametrize("name", sorted(CASES))
def test_root_inside_equals_the_oracle_prune(name):
    pb, pr = CASES[name]
    mats = MR.oracle_matrices(pb, pr, O)
    mults = [1.0] if pr.multipliers is None else list(pr.multipliers)
    for f in range(pb.n_families):
        ud = MR.updown_family(pb, pr, mats, f, 0.95)
        for k, m in enumerate(mults):
            _close(ud["root_inside"][k], O.prune(pb, pr, f, mult=m))


def test_failed_family_is_nan_and_minus_one():
    pb, pr = CASES["binary5"]
    pr = P.Params(lambdas=np.array([5.0]), prior=pr.prior)           # saturated: every row s >= 1 of every matrix is 0
    ud = MR.updown_family(pb, pr, MR.oracle_matrices(pb, pr, O), 0, 0.95)
    assert ud["failed"] == 1 and np.isnan(ud["log_evidence"])
    assert np.all(np.isnan(ud["mean"])) and np.all(ud["mode"] == -1) and np.all(ud["lo"] == -1) and np.all(ud["hi"] == -1)


def test_library_exports_the_entry_point():
    from cafexp_amd import capi
    assert "cafe_marginal_reconstruct" in capi.EXPORTS
    assert getattr(capi.load(), "cafe_marginal_reconstruct") is not None
    assert hasattr(capi.Context, "marginal_reconstruct")


def test_driver_usage_names_the_flag():
    exe = os.path.join(ROOT, "cafexp_amd", "host", "cafexp_hip")
    assert os.path.exists(exe), "cafexp_hip missing: run __graft_entry__.build()"
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2
    assert "--reconstruct-marginal" in r.stderr
