"""cafexp_hip --gain NU --gain-dense --leaf-predictive on the drawn table of tests/test_gain_driver.py: Gain_leaf_predictive.tab is
cafe_gain_leaf_predictive's arrays at the same rates, cell for cell at the six printed digits, and the JSON line's sum of log p_obs
is the arrays' (1e-8 relative, test_leaf_predictive_driver's bound).  Without --gain-dense the option stays refused."""
import json
import os
import subprocess

import numpy as np
import pytest

import bd_lm_ref as R
from cafexp_amd import problem as P
from test_gain_driver import ABSENT, DRIVER, LAM, M, NU, RR, _problem, draw_table
from test_leaf_predictive_driver import _read_tab

FAMILIES = 80


@pytest.mark.gpu
def test_the_table_is_the_bindings_arrays(tmp_path):
    from cafexp_amd import capi
    assert os.path.exists(DRIVER), "cafexp_hip missing: run __graft_entry__.build()"
    counts = draw_table()[:FAMILIES]
    tree, fams, out = tmp_path / "tree.txt", tmp_path / "families.txt", tmp_path / "out"
    tree.write_text(R.NEWICK + "\n")
    fams.write_text("Desc\tFamily ID\t" + "\t".join(R.SPECIES) + "\n" + "".join("(null)\tf%d\t%s\n" % (i, "\t".join(map(str, c))) for i, c in enumerate(counts)))
    common = [DRIVER, "-t", str(tree), "-i", str(fams), "-z", "-l", str(LAM), "--gain", str(NU), "--leaf-predictive", "--root-absent", str(ABSENT),
              "--sizes", "%d,%d" % (M, RR), "-o", str(out)]
    refused = subprocess.run(common, capture_output=True, text=True, timeout=300)
    assert refused.returncode == 1 and "the posterior reports are not ported to the gain model" in refused.stderr
    r = subprocess.run(common + ["--gain-dense"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    js = json.loads(r.stdout.strip().splitlines()[-1])
    assert sorted(js["leaf_predictive"]) == ["failed_cells", "log_pseudo_likelihood", "outliers", "seconds"] and js["leaf_predictive"]["failed_cells"] == 0
    pb = _problem(counts)
    ctx = capi.Context(pb)
    try:
        got = ctx.gain_leaf_predictive(P.Params(lambdas=np.ones(1), prior=P.prior_uniform(RR)), np.arange(FAMILIES), [LAM], [LAM], [NU], ABSENT)
    finally:
        ctx.close()
    assert not np.isnan(got["p_obs"]).any()
    head, rows = _read_tab(str(out / "Gain_leaf_predictive.tab"))
    assert sorted(head[1:]) == sorted(pb.taxa) and [r[0] for r in rows] == ["f%d" % i for i in range(FAMILIES)]
    for f in range(FAMILIES):
        for j, t in enumerate(list(pb.taxa).index(s) for s in head[1:]):
            want = (got["mean"][f, t], got["sd"][f, t], got["p_below"][f, t] + got["p_obs"][f, t], got["p_obs"][f, t] + got["p_above"][f, t])
            assert rows[f][1 + j] == "%.6g:%.6g:%.6g:%.6g" % want, (f, t)
    total = np.log(got["p_obs"][got["p_obs"] > 0]).sum()
    assert abs(js["leaf_predictive"]["log_pseudo_likelihood"] - total) <= 1e-8 * abs(total)
    assert os.path.exists(out / "Gain_leaf_outliers.tab") and os.path.exists(out / "Gain_species_fit.tab") and not os.path.exists(out / "Gain_imputed_counts.tab")
