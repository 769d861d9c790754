"""cafexp_hip --gain NU --gain-dense --reconstruct-marginal on the drawn table of tests/test_gain_driver.py writes
Gain_posterior_sizes.tab and Gain_posterior_change.tab; a family's lines are cafe_gain_marginal_dense's arrays at the same rates at the
printed digits, every leaf column by its name.  Without --gain-dense the option stays refused."""
import json
import os
import subprocess

import numpy as np
import pytest

import bd_lm_ref as R
from cafexp_amd import problem as P
from test_gain_driver import ABSENT, DRIVER, LAM, M, NU, RR, _problem, draw_table
from test_leaf_predictive_driver import _read_tab

FAMILIES, LEVEL, SPOT = 80, 0.9, 7


@pytest.mark.gpu
def test_both_tables_are_the_bindings_arrays(tmp_path):
    from cafexp_amd import capi
    assert os.path.exists(DRIVER), "cafexp_hip missing: run __graft_entry__.build()"
    counts = draw_table()[:FAMILIES]
    tree, fams, out = tmp_path / "tree.txt", tmp_path / "families.txt", tmp_path / "out"
    tree.write_text(R.NEWICK + "\n")
    fams.write_text("Desc\tFamily ID\t" + "\t".join(R.SPECIES) + "\n" + "".join("(null)\tf%d\t%s\n" % (i, "\t".join(map(str, c))) for i, c in enumerate(counts)))
    common = [DRIVER, "-t", str(tree), "-i", str(fams), "-z", "-l", str(LAM), "--gain", str(NU), "--reconstruct-marginal", str(LEVEL), "--root-absent",
              str(ABSENT), "--sizes", "%d,%d" % (M, RR), "-o", str(out)]
    refused = subprocess.run(common, capture_output=True, text=True, timeout=300)
    assert refused.returncode == 1 and ("the reconstructions are not ported to the gain model: --reconstruct, --reconstruct-marginal and --sample-histories "
                                        "are not supported with --gain / --estimate-gain") in refused.stderr
    r = subprocess.run(common + ["--gain-dense"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    js = json.loads(r.stdout.strip().splitlines()[-1])
    assert js["marginal"]["failed"] == 0 and js["marginal"]["level"] == LEVEL
    pb = _problem(counts)
    ctx = capi.Context(pb)
    try:
        got = ctx.gain_marginal_dense(P.Params(lambdas=np.ones(1), prior=P.prior_uniform(RR)), [SPOT], [LAM], [LAM], [NU], ABSENT, LEVEL)
    finally:
        ctx.close()
    root = int(np.where(pb.parent < 0)[0][0])
    cells = {"Gain_posterior_sizes.tab": ["%.6g:%d:%d-%d" % (got["mean"][0, v], got["mode"][0, v], got["lo"][0, v], got["hi"][0, v]) for v in range(pb.n_nodes)],
             "Gain_posterior_change.tab": ["-" if v == root else "%.6g:%.6g" % (got["p_decrease"][0, v], got["p_increase"][0, v]) for v in range(pb.n_nodes)]}
    for name, want in cells.items():
        head, rows = _read_tab(str(out / name))
        assert len(rows) == FAMILIES and rows[SPOT][0] == "f%d" % SPOT and len(head) == 1 + pb.n_nodes
        for v, t in enumerate(pb.leaf_taxon):
            if t >= 0:
                assert rows[SPOT][1 + [h.split("<")[0] for h in head[1:]].index(pb.taxa[t])] == want[v], (name, pb.taxa[t])
