"""cafexp_hip --gain NU --gain-posterior --gain-dense: test_gain_posterior_driver's run through cafe_gain_posterior_dense.  Both
report files against the dense binding's arrays, that test's bounds: 5e-6 relative (6 printed digits) and 1e-9 of the sums."""
import json
import os
import subprocess

import numpy as np
import pytest

import bd_lm_ref as R
import marginal_ref as MR
from cafexp_amd import problem as P
from test_events_driver import _read_tab, _reverse_level_order
from test_gain_driver import ABSENT, DRIVER, LAM, M, NU, RR, _problem, draw_table
from test_gain_posterior_driver import FAMILIES, _cells


@pytest.mark.gpu
def test_both_files_are_the_dense_bindings_arrays(tmp_path):
    from cafexp_amd import capi
    assert os.path.exists(DRIVER), "cafexp_hip missing: run __graft_entry__.build()"
    counts = draw_table()[:FAMILIES]
    tree, fams, out = tmp_path / "tree.txt", tmp_path / "families.txt", tmp_path / "out"
    tree.write_text(R.NEWICK + "\n")
    fams.write_text("Desc\tFamily ID\t" + "\t".join(R.SPECIES) + "\n" + "".join("(null)\tf%d\t%s\n" % (i, "\t".join(map(str, c))) for i, c in enumerate(counts)))
    r = subprocess.run([DRIVER, "-t", str(tree), "-i", str(fams), "-z", "-l", str(LAM), "--gain", str(NU), "--gain-posterior", "--gain-dense", "--root-absent",
                        str(ABSENT), "--sizes", "%d,%d" % (M, RR), "-o", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    js = json.loads(r.stdout.strip().splitlines()[-1])
    assert js["gain_posterior_path"] == "cafe_gain_posterior_dense" and js["families"] == FAMILIES and js["nu"] == NU
    pb = _problem(counts)
    pr = P.Params(lambdas=np.ones(1), prior=P.prior_uniform(RR))
    ctx = capi.Context(pb)
    try:
        got = ctx.gain_posterior_dense(pr, np.arange(FAMILIES), [LAM], [LAM], [NU], ABSENT)
    finally:
        ctx.close()
    assert np.isfinite(got["lnl"]).all()
    order, root = _reverse_level_order(pb), MR.root_of(pb)
    branches, n = [v for v in order if v != root], pb.n_nodes
    head, rows = _read_tab(str(out / "Gain_origins.tab"))
    assert len(head) == 2 * n and [r[0] for r in rows] == ["f%d" % i for i in range(FAMILIES)]
    printed = {k: np.full((FAMILIES, n), np.nan) for k in ("p_absent", "mean", "p_gain", "p_loss")}
    for f in range(FAMILIES):
        nodes, edges = _cells(rows[f], 1, n), _cells(rows[f], 1 + n, n - 1)
        printed["p_absent"][f, order], printed["mean"][f, order] = nodes[:, 0], nodes[:, 1]
        printed["p_gain"][f, branches], printed["p_loss"][f, branches] = edges[:, 0], edges[:, 1]
    for key, values in printed.items():
        assert np.array_equal(np.isnan(values), np.isnan(got[key])), key
        keep = ~np.isnan(values)
        assert np.max(np.abs(values[keep] - got[key][keep]) - 5e-6 * np.abs(got[key][keep])) <= 1e-300, key
    thead, trows = _read_tab(str(out / "Gain_branch_origins.tab"))
    assert "%d families; 0 failed" % FAMILIES in thead[5]
    for row, v in zip(trows[:-1], branches):
        for value, want in ((float(row[1]), got["p_gain"][:, v]), (float(row[2]), got["p_loss"][:, v]), (float(row[3]), 1 - got["p_absent"][:, v])):
            assert abs(value - want.sum()) <= 1e-9 * np.abs(want).sum() + 1e-300, (v, row)
        assert float(row[4]) == (got["p_gain"][:, v] > 0.5).sum()
    assert abs(float(trows[-1][2]) - got["p_absent"][:, root].sum()) <= 1e-9 * FAMILIES
    assert js["families_with_a_likely_origin"] == (np.nanmax(got["p_gain"], axis=1) > 0.5).sum() >= 1
