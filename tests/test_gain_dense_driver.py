"""cafexp_hip --estimate-gain --gain-dense: the search of tests/test_gain_driver.py's drawn table scored through cafe_score_gain
ends where the default path's ends -- -lnL to 1e-9 relative, lambda and nu to 1e-6, the family likelihoods to 1e-10 -- and the
flag alone, without a gain option, is refused with its reason."""
import json
import subprocess

import numpy as np
import pytest

import bd_lm_ref as R
from test_gain_driver import ABSENT, DRIVER, M, RR, draw_table


def _fit(tmp_path, fams, name, *flags):
    out = tmp_path / name
    r = subprocess.run([DRIVER, "-t", str(tmp_path / "tree.txt"), "-i", str(fams), "-z", "--estimate-gain", "--root-absent", str(ABSENT), "--sizes",
                        "%d,%d" % (M, RR), "-s", "3", "-o", str(out), *flags], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rows = (out / "Gain_family_likelihoods.txt").read_text().splitlines()[1:]
    return json.loads(r.stdout.strip().splitlines()[-1]), np.array([float(ln.split("\t")[1]) for ln in rows])


@pytest.mark.gpu
def test_the_dense_search_ends_where_the_per_family_search_ends(tmp_path):
    counts = draw_table()
    (tmp_path / "tree.txt").write_text(R.NEWICK + "\n")
    fams = tmp_path / "families.txt"
    fams.write_text("Desc\tFamily ID\t" + "\t".join(R.SPECIES) + "\n" + "".join("(null)\tf%d\t%s\n" % (i, "\t".join(map(str, c))) for i, c in enumerate(counts)))
    (plain, plain_lnl), (dense, dense_lnl) = _fit(tmp_path, fams, "plain"), _fit(tmp_path, fams, "dense", "--gain-dense")
    print("per family: -lnL %.12f lambda %.10g nu %.10g, %d calls; dense: -lnL %.12f lambda %.10g nu %.10g, %d calls"
          % (plain["neg_lnl"], plain["lambda"][0], plain["nu"], plain["calls"], dense["neg_lnl"], dense["lambda"][0], dense["nu"], dense["calls"]))
    for key in ("neg_lnl", "neg_lnl_without_gain"):
        assert abs(dense[key] - plain[key]) <= 1e-9 * abs(plain[key]), key
    assert abs(dense["lambda"][0] - plain["lambda"][0]) <= 1e-6 * plain["lambda"][0]
    assert abs(dense["nu"] - plain["nu"]) <= 1e-6 * plain["nu"]
    assert len(dense_lnl) == len(counts) + 1 and np.allclose(dense_lnl, plain_lnl, rtol=1e-10, atol=0)


def test_the_flag_needs_a_gain_option(tmp_path):
    r = subprocess.run([DRIVER, "-t", str(tmp_path / "none"), "-i", str(tmp_path / "none"), "--gain-dense"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--gain-dense scores the gain model's shared rates on the dense prune: give --gain NU or --estimate-gain with it" in r.stderr
