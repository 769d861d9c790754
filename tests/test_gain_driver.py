"""cafexp_hip --estimate-gain on a table drawn from the gain model itself: about 400 families drawn by numpy from the reference
matrices of tests/gain_ref.py on the six-taxon tree of tests/bd_lm_ref.py (fixed seed, lambda = mu = 0.012, nu / lambda = 0.5,
root absent with probability 0.3, otherwise a size uniform on 1..R), the all-zero families dropped as a table drops them.

The driver's fit is held against the same objective written in numpy -- the likelihood conditional on a family being seen, sum
rule -- searched by scipy's Nelder-Mead from the driver's own starts: the driver's -lnL must not end above scipy's by more than
1e-6 relative, its printed optimum rescored in numpy agrees to 1e-9, and the gain fit is not worse than the nu = 0 fit it
extends.  How well nu is recovered is reported in DESIGN section 8, not asserted."""
import json
import os
import subprocess

import numpy as np
import pytest

import bd_lm_ref as R
import gain_ref as G
import marginal_ref as MR
from cafexp_amd import problem as P

HERE = os.path.dirname(os.path.abspath(__file__))
DRIVER = os.path.join(os.path.dirname(HERE), "cafexp_amd", "host", "cafexp_hip")
M, RR = 30, 8
LAM, NU, ABSENT, DRAWN = 0.012, 0.006, 0.3, 545


def _problem(counts):
    return P.build_problem(P.parse_newick(R.NEWICK), R.SPECIES, ["f%d" % i for i in range(len(counts))], counts, root_filter=False,
                           max_family_size=M, max_root_family_size=RR)


def draw_table():
    """counts[F][6] of the families that at least one species shows"""
    rng = np.random.default_rng(20)
    pb = _problem(np.zeros((1, 6), dtype=np.int32))
    mats = G.matrices(pb, [LAM], [LAM], [NU])
    ch, root = MR.children_of(pb), MR.root_of(pb)
    rows = []
    for _ in range(DRAWN):
        size = {root: 0 if rng.random() < ABSENT else int(rng.integers(1, RR + 1))}
        stack, counts = [root], np.zeros(6, dtype=np.int32)
        while stack:
            v = stack.pop()
            for u in ch[v]:
                p = mats[u][size[v]]
                size[u] = int(rng.choice(len(p), p=p / p.sum()))
                stack.append(u)
            if pb.leaf_taxon[v] >= 0:
                counts[pb.leaf_taxon[v]] = size[v]
        if counts.any():
            rows.append(counts)
    return np.array(rows, dtype=np.int32)


class Objective:
    """-sum_f w_f lnL_f + F log(1 - exp(lnL_absent)) over the distinct families of a table, every family pruned at once"""

    def __init__(self, counts):
        self.distinct, self.weight = np.unique(counts, axis=0, return_counts=True)
        self.F = len(counts)
        self.pb = _problem(np.concatenate([self.distinct, np.zeros((1, 6), dtype=np.int32)]))
        self.prior = P.prior_uniform(RR)
        self.ch, self.root = MR.children_of(self.pb), MR.root_of(self.pb)

    def lnl(self, lam, mu, nu):
        from scipy.special import logsumexp
        pb = self.pb
        mats = G.matrices(pb, [lam], [mu], [nu])
        fac = {}
        for v in range(pb.n_nodes):                          # children come before their parents in a problem's node order
            if v == self.root:
                continue
            assert all(u in fac for u in self.ch[v])
            rows = (RR if pb.parent[v] == self.root else M) + 1
            if pb.leaf_taxon[v] >= 0:
                fac[v] = mats[v][:rows][:, pb.counts[:, pb.leaf_taxon[v]]]
            else:
                fac[v] = mats[v][:rows, :M + 1] @ np.prod([fac[u][:M + 1] for u in self.ch[v]], axis=0)
        L = np.prod([fac[u][:RR + 1] for u in self.ch[self.root]], axis=0)
        mass = np.concatenate([[ABSENT], (1 - ABSENT) * self.prior.astype(np.float64)])
        with np.errstate(divide="ignore"):
            return logsumexp(np.log(L) + np.log(mass)[:, None], axis=0)

    def __call__(self, lam, nu):
        if not (lam > 0 and nu >= 0):
            return np.inf
        v = self.lnl(lam, lam, nu)
        if not np.isfinite(v[:-1]).all() or v[-1] >= 0:
            return np.inf
        return float(-(self.weight * v[:-1]).sum() + self.F * np.log(-np.expm1(v[-1])))


@pytest.mark.gpu
def test_the_gain_search_against_scipy_on_the_numpy_objective(tmp_path):
    from scipy.optimize import minimize
    assert os.path.exists(DRIVER), "cafexp_hip missing: run __graft_entry__.build()"
    counts = draw_table()
    assert 350 <= len(counts) <= 450 and counts.max() <= M - 2
    one_clade = ((counts[:, :2].sum(axis=1) == 0) | (counts[:, 2:].sum(axis=1) == 0)).sum()
    assert one_clade >= 20                                   # families a model without gain cannot explain unless the root held them
    tree, fams = tmp_path / "tree.txt", tmp_path / "families.txt"
    tree.write_text(R.NEWICK + "\n")
    fams.write_text("Desc\tFamily ID\t" + "\t".join(R.SPECIES) + "\n" + "".join("(null)\tf%d\t%s\n" % (i, "\t".join(map(str, c))) for i, c in enumerate(counts)))
    out = tmp_path / "out"
    r = subprocess.run([DRIVER, "-t", str(tree), "-i", str(fams), "-z", "--estimate-gain", "--root-absent", str(ABSENT), "--sizes", "%d,%d" % (M, RR), "-s", "3",
                        "-o", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    js = json.loads(r.stdout.strip().splitlines()[-1])
    print(js)
    assert js["model"] == "Gain" and js["root_rule"] == "sum" and js["conditional"] is True and js["families"] == len(counts)
    assert js["max_family_size"] == M and js["max_root_family_size"] == RR and js["mu"] == js["lambda"]

    obj = Objective(counts)
    assert js["distinct_families"] == len(obj.distinct)
    # the printed optima rescored
    for neg, lam, nu in ((js["neg_lnl"], js["lambda"][0], js["nu"]), (js["neg_lnl_without_gain"], js["lambda_without_gain"][0], 0.0)):
        mine = obj(lam, nu)
        print("driver %.12f numpy %.12f at lambda %.10g nu %.10g" % (neg, mine, lam, nu))
        assert abs(mine - neg) <= 1e-9 * abs(neg)
    # scipy from the driver's starts: the same nesting
    opts = dict(xatol=1e-10, fatol=1e-9, maxiter=2000, maxfev=4000)
    first = minimize(lambda x: obj(x[0], 0.0), js["start_without_gain"], method="Nelder-Mead", options=opts)
    assert js["start"] == [js["lambda_without_gain"][0], js["lambda_without_gain"][0] / 10]
    second = minimize(lambda x: obj(x[0], x[1]), js["start"], method="Nelder-Mead", options=opts)
    print("scipy: without gain %.10f at %s, with gain %.10f at %s (%d + %d evaluations); driver %d calls"
          % (first.fun, first.x, second.fun, second.x, first.nfev, second.nfev, js["calls"]))
    assert js["neg_lnl_without_gain"] <= first.fun + 1e-6 * abs(first.fun)
    assert js["neg_lnl"] <= second.fun + 1e-6 * abs(second.fun)
    assert js["neg_lnl"] <= js["neg_lnl_without_gain"]
    assert abs(js["lr_statistic"] - 2 * (js["neg_lnl_without_gain"] - js["neg_lnl"])) <= 1e-9 * max(1.0, js["lr_statistic"])
    print("recovery: nu %.6g (drawn with %.6g), lambda %.6g (drawn with %.6g), LR statistic %.3f" % (js["nu"], NU, js["lambda"][0], LAM, js["lr_statistic"]))

    text = (out / "Gain_results.txt").read_text()
    for line in ("Root rule: sum", "Root absent: 0.2999999", "Likelihood: conditional on the family being seen in at least one species",
                 "Without gain (-lnL): ", "Likelihood ratio statistic: ", "r (Nu / Lambda): "):
        assert line in text, text
    rows = (out / "Gain_family_likelihoods.txt").read_text().splitlines()
    assert len(rows) == len(counts) + 2 and rows[-1].startswith("(absent)\t")
    got = np.array([float(ln.split("\t")[1]) for ln in rows[1:-1]])
    want = obj.lnl(js["lambda"][0], js["lambda"][0], js["nu"])
    index = {tuple(c): i for i, c in enumerate(obj.distinct)}
    assert np.allclose(got, [want[index[tuple(c)]] for c in counts], rtol=1e-10, atol=0)
    assert abs(float(rows[-1].split("\t")[1]) - want[-1]) <= 1e-10 * abs(want[-1])
