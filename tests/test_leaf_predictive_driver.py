"""cafexp_hip --leaf-predictive on synth20: after the search the driver writes <Model>_leaf_predictive.tab (mean:sd:p_low:p_high
per family and species, "-" for a cell without mass), <Model>_leaf_outliers.tab (the cells whose two-sided p, Holm-adjusted over
every finite cell of the table, is at most -P, most extreme first) and <Model>_species_fit.tab.  All three are recomputed from the
binding's own cafe_leaf_predictive arrays at the printed optimum: the cells printed the same way (equal strings), the outliers as
the set and order Holm's step selects in numpy (at -P 0.05, where this simulated table has few or none, and at -P 1, which lists
every cell), the per-species sums to 1e-8 relative as tests/test_events_driver.py holds its
totals."""
import json
import os
import subprocess

import numpy as np
import pytest

from cafexp_amd import problem as P
from helpers import DATA, read, table

HERE = os.path.dirname(os.path.abspath(__file__))
DRIVER = os.path.join(os.path.dirname(HERE), "cafexp_amd", "host", "cafexp_hip")
COMMON = ["-t", os.path.join(DATA, "synth20_tree.txt"), "-i", os.path.join(DATA, "synth20_families.txt"), "-s", "7", "--leaf-predictive"]


def _read_tab(path):
    with open(path) as f:
        rows = [ln.rstrip("\n").split("\t") for ln in f if ln.strip()]
    return rows[0], rows[1:]


def _holm(p):
    order = np.argsort(p, kind="stable")
    adj, run = np.empty(len(p)), 0.0
    for r, i in enumerate(order):
        run = max(run, min(1.0, (len(p) - r) * p[i]))
        adj[i] = run
    return adj


@pytest.mark.gpu
@pytest.mark.parametrize("extra,model,threshold", [([], "Base", "0.05"), (["-k", "2"], "Gamma", "1")])
def test_the_tables_are_the_bindings_arrays_at_the_printed_optimum(tmp_path, extra, model, threshold):
    from cafexp_amd import capi
    assert os.path.exists(DRIVER), "cafexp_hip missing: run __graft_entry__.build()"
    r = subprocess.run([DRIVER] + COMMON + ["-P", threshold, "-o", str(tmp_path)] + extra, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    js = json.loads(r.stdout.strip().splitlines()[-1])
    assert sorted(js["leaf_predictive"]) == ["failed_cells", "log_pseudo_likelihood", "outliers", "seconds"]
    assert js["leaf_predictive"]["failed_cells"] == 0 and js["leaf_predictive"]["seconds"] >= 0

    species, ids, counts = table("synth20_families.txt")
    pb = P.build_problem(P.parse_newick(read("synth20_tree.txt")), species, ids, counts)
    assert pb.n_families == js["n_families"] and pb.max_family_size == js["max_family_size"]
    pr = P.Params(lambdas=np.array(js["lambda"]), prior=P.prior_uniform(pb.max_root_family_size))
    K = 1
    if model == "Gamma":
        K = 2
        pr.multipliers, pr.cat_probs = np.array(js["multipliers"]), np.full(2, 0.5)
    ctx = capi.Context(pb, max_categories=K)
    try:
        got = ctx.leaf_predictive(pr, alpha=js.get("alpha", 1.0))
    finally:
        ctx.close()
    assert not np.isnan(got["p_obs"]).any()
    p_low, p_high = got["p_below"] + got["p_obs"], got["p_obs"] + got["p_above"]

    head, rows = _read_tab(os.path.join(str(tmp_path), model + "_leaf_predictive.tab"))
    assert head[0] == "FamilyID" and sorted(head[1:]) == sorted(species) and [r[0] for r in rows] == list(pb.family_ids)
    col = [list(species).index(s) for s in head[1:]]         # the driver's species order -> the binding's columns
    for f in range(pb.n_families):
        for j, t in enumerate(col):
            assert rows[f][1 + j] == "%.6g:%.6g:%.6g:%.6g" % (got["mean"][f, t], got["sd"][f, t], p_low[f, t], p_high[f, t]), (f, t)

    # Holm over all cells, in the driver's table order (family, then its species order)
    cells = [(f, t) for f in range(pb.n_families) for t in col]
    p = np.array([min(1.0, 2 * min(p_low[c], p_high[c])) for c in cells])
    adj = _holm(p)
    picked = [i for i in sorted(range(len(cells)), key=lambda i: (adj[i], p[i], i)) if adj[i] <= float(threshold)]
    ohead, orows = _read_tab(os.path.join(str(tmp_path), model + "_leaf_outliers.tab"))
    assert ohead[:8] == ["#FamilyID", "Species", "Observed", "Mean", "SD", "Direction", "P", "HolmP"] and "Holm over %d cells" % len(cells) in ohead[8]
    print("%s: %d outliers at %s of %d cells" % (model, len(picked), threshold, len(cells)))
    assert len(orows) == len(picked) == js["leaf_predictive"]["outliers"]
    assert len(picked) == len(cells) if threshold == "1" else len(picked) < len(cells)      # -P 1 lists every cell, in Holm's order
    for row, i in zip(orows, picked):
        f, t = cells[i]
        want = [pb.family_ids[f], species[t], "%d" % pb.counts[f, t], "%.6g" % got["mean"][f, t], "%.6g" % got["sd"][f, t],
                "low" if p_low[f, t] <= p_high[f, t] else "high", "%.6g" % p[i], "%.6g" % adj[i]]
        assert row == want, (row, want)

    shead, srows = _read_tab(os.path.join(str(tmp_path), model + "_species_fit.tab"))
    assert shead == ["#Species", "Cells", "MeanZ", "OutliersLow", "OutliersHigh", "SumLogPObs"] and [r[0] for r in srows] == head[1:]
    total = 0.0
    for row, t in zip(srows, col):
        ok = got["sd"][:, t] > 0
        z = ((pb.counts[:, t] - got["mean"][:, t])[ok] / got["sd"][ok, t]).mean()
        mine = [i for i in picked if cells[i][1] == t]
        low = sum(1 for i in mine if p_low[cells[i]] <= p_high[cells[i]])
        logp = np.log(got["p_obs"][:, t][got["p_obs"][:, t] > 0]).sum()
        total += logp
        assert int(row[1]) == pb.n_families and int(row[3]) == low and int(row[4]) == len(mine) - low, row
        assert abs(float(row[2]) - z) <= 5e-6 * abs(z) + 1e-10 and abs(float(row[5]) - logp) <= 1e-8 * abs(logp), (row, z, logp)
    assert abs(js["leaf_predictive"]["log_pseudo_likelihood"] - total) <= 1e-8 * abs(total)


def test_the_driver_refuses_what_does_not_combine(tmp_path):
    assert os.path.exists(DRIVER), "cafexp_hip missing: run __graft_entry__.build()"
    common = COMMON + ["-P", "0.05", "-o", str(tmp_path / "out")]
    for extra, message in ((["-b"], "-b is not supported with it"), (["--gpus", "2"], "--gpus is not supported with it"),
                           (["--simulate", "10", "-l", "0.01"], "--simulate is not supported with it")):
        r = subprocess.run([DRIVER] + common + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--leaf-predictive" in r.stderr and message in r.stderr, (extra, r.stderr)
    assert not os.path.exists(str(tmp_path / "out"))
