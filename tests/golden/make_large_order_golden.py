#!/usr/bin/env python3
"""Generates tests/golden/ref_large_order.json from the REAL reference: fixtures at matrix orders above 751, up to the
largest order the library accepts (bd_matrix_max_order() = 2048).  Under the reference's size rules (user_data.cpp:45-46:
R = rint(1.25 m), M = m + max(50, m / 5)) a table whose largest count is m has order N = max(M, R) + 1:
m = 900 -> N = 1126, m = 1637 -> N = 2047 (the largest a family table can reach; m = 1638 gives 2049).

Run in the build container only (needs /root/reference and `make -C oracle ref`):
    python tests/golden/make_large_order_golden.py
Every value is printed by oracle/_ref/ref_harness (our driver around the reference's own functions) with 17 significant
digits; the fixture holds inputs + expected outputs only.  The reference builds a matrix as O(N^3) log-space sums on one
thread per matrix, so the jobs run side by side.  Measured on 8 cores: 16 minutes for the whole file (the base score at N = 2047 alone takes 15).

  matrices  n = 1025 (the first order where the scorer's two-pool K1 launch uses 20 columns per lane) at three
            (lambda * m_k, t) and n = 2047 at two: rows 1, 2, M, R, N-1 and the diagonal (M, R of the table whose
            order is n) thinned to every 64th entry plus their band edges, and a fixed sample of entries: the band edges of a
            grid of rows (first / last column with an entry above 1e-290), the deep tail (entries between 1e-300 and
            1e-280) and seeded random entries
  scores    large6_*  6 taxa, 14 families, one family with a tip at 900 (M = 1080, R = 1125, N = 1126): gamma K = 4 per
                      family and category, the base model, a lambda tree (two rates) + a 3-tap error model
            huge6_base  6 taxa, 10 families, one tip at 1637 (M = 1964, R = 2046, N = 2047): the base model
"""
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import oracle as O  # noqa: E402
import numpy as np  # noqa: E402
from cafexp_amd import synth  # noqa: E402
from cafexp_amd.problem import max_sizes  # noqa: E402

D = os.path.join(HERE, "data")
OUT = os.path.join(HERE, "ref_large_order.json")

# (n, max count of the table whose order is n): rows M and R are the contraction / root extents of such a table
ORDERS = {1025: 819, 2047: 1637}


def matrix_pairs():
    _, mult = O.discrete_gamma(4, 0.8)
    return [(1025, 0.002 * float(mult[0]), 61.337), (1025, 0.002 * float(mult[3]), 7.25), (1025, 0.0011, 23.904),
            (2047, 0.002 * float(mult[0]), 61.337), (2047, 0.0013, 9.75)]


def write_table(name, tree, counts):
    species = [l.name for l in tree.leaves()]
    with open(os.path.join(D, name + "_tree.txt"), "w") as f:
        f.write(synth.to_newick(tree) + "\n")
    with open(os.path.join(D, name + "_families.txt"), "w") as f:
        f.write("Desc\tFamily ID\t" + "\t".join(species) + "\n")
        for i, row in enumerate(counts):
            f.write("(null)\tfam%04d\t" % i + "\t".join(str(int(x)) for x in row) + "\n")


def write_lambda_tree(name, tree):
    cands = [n for n in tree.postorder() if not n.is_leaf and n.parent is not None and len(n.leaves()) >= 2]
    pick = min(cands, key=lambda n: len(n.leaves()))
    marked = {id(x) for x in pick.postorder()}

    def rec(n):
        idx = 2 if id(n) in marked else 1
        if n.is_leaf:
            return "%s:%d" % (n.name, idx)
        return "(" + ",".join(rec(c) for c in n.children) + ")" + (":%d" % idx if n.parent is not None else "")
    with open(os.path.join(D, name + "_lambda_tree.txt"), "w") as f:
        f.write(rec(tree) + ";\n")


def write_tables():
    """Generated the way make_n751_golden.write_big12 does it: family 0 is a large, slowly evolving family with one tip at
    exactly the table's maximum; family 1 a second large one; family 2 has an outlying tip."""
    for name, seed, n_fam, mx in (("large6", 1126, 14, 900), ("huge6", 2047, 10, 1637)):
        rng = np.random.default_rng(seed)
        tree = synth.yule_tree(6, rng)
        counts = synth.simulate_families(tree, n_fam, 0.002, rng, max_count=mx, root_cap=300)
        big = synth.simulate_families(tree, 1, 0.002 / 20.0, rng, max_count=mx, root_cap=mx, root_p=1e-9)
        counts[0] = big[0]
        counts[0, int(np.argmax(counts[0]))] = mx
        counts[1] = np.maximum(1, (counts[0] * 0.55).astype(np.int64))
        counts[2, 0] = 130
        assert int(counts.max()) == mx
        write_table(name, tree, counts)
        if name == "large6":
            write_lambda_tree(name, tree)
    with open(os.path.join(D, "errormodel_900.txt"), "w") as f:
        f.write("maxcnt:900\ncntdiff -1 0 1\n0 0.00 0.95 0.05\n1 0.05 0.9 0.05\n450 0.08 0.84 0.08\n900 0.1 0.8 0.1\n")


def sample_entries(m):
    """[s, c, value] triples: per row of a grid the first and last column with an entry above 1e-290 (the band edges), the
    deep tail next to the last one, and 40 seeded random entries."""
    n = m.shape[0]
    picks = set()
    for s in sorted(set(np.linspace(1, n - 1, 12).astype(int).tolist())):
        big = np.nonzero(m[s] > 1e-290)[0]
        if len(big):
            lo, hi = int(big[0]), int(big[-1])
            picks.update((s, c) for c in (lo, lo + 1, hi - 1, hi, hi + 1, hi + 2) if 0 <= c < n)
        tail = np.nonzero((m[s] > 1e-300) & (m[s] < 1e-280))[0]
        if len(tail):
            picks.update((s, int(c)) for c in tail[:: max(1, len(tail) // 3)][:4])
    rng = np.random.default_rng(n)
    picks.update((int(s), int(c)) for s, c in zip(rng.integers(1, n, 40), rng.integers(0, n, 40)))
    return [[s, c, float(m[s, c])] for s, c in sorted(picks)]


def thin(v):
    """[index, value] pairs of a row (or the diagonal): every 64th entry, the last one, and the band edges -- the first
    and last entry above 1e-290, their neighbours and the largest entry."""
    v = np.asarray(v)
    n = len(v)
    picks = set(range(0, n, 64)) | {n - 1, int(np.argmax(v))}
    big = np.nonzero(v > 1e-290)[0]
    if len(big):
        lo, hi = int(big[0]), int(big[-1])
        picks.update(c for c in (lo - 1, lo, lo + 1, hi - 1, hi, hi + 1, hi + 2) if 0 <= c < n)
    return [[c, float(v[c])] for c in sorted(picks)]


def write_fixture(g):
    """One line per matrix and per score: a reviewable file (a number per line would be 40 000 lines)."""
    with open(OUT, "w") as f:
        f.write("{\n")
        f.write("".join("%s:%s,\n" % (json.dumps(k), json.dumps(g[k])) for k in ("generator", "source")))
        f.write('"matrices":[\n' + ",\n".join(json.dumps(m, separators=(",", ":")) for m in g["matrices"]) + "\n],\n")
        f.write('"scores":{\n' + ",\n".join("%s:%s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in g["scores"].items()) + "\n}\n}\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes", flush=True)


def one_matrix(job):
    n, lam, t = job
    r = O.ref("matrix", n=n, **{"lambda": repr(lam), "t": repr(t)})
    m = np.array(r["values"]).reshape(n, n)
    M, R = max_sizes(np.array([[ORDERS[n]]]))
    assert max(M, R) + 1 == n
    rows = sorted({1, 2, M, R, n - 1})
    print("ref matrix n=%d lambda=%r t=%r done" % (n, lam, t), flush=True)
    return {"n": n, "lambda": lam, "t": t, "M": M, "R": R, "diag": thin(m.diagonal()), "rows": {str(i): thin(m[i]) for i in rows},
            "sample": sample_entries(m)}


def entry(kv, r):
    e = {"args": {k: (os.path.basename(v) if isinstance(v, str) and os.sep in v else v) for k, v in kv.items()}}
    e.update(r)
    e.pop("seconds", None)               # (wall time and OpenMP threads: would make the file differ run to run, machine to machine)
    e.pop("threads", None)
    return e


def score_jobs():
    data = lambda n: os.path.join(D, n)  # noqa: E731
    return {
        "large6_gamma_k4": dict(tree=data("large6_tree.txt"), families=data("large6_families.txt"), per_family=1, model="gamma", k=4,
                                alpha=0.8, **{"lambda": 0.002}),
        "large6_base": dict(tree=data("large6_tree.txt"), families=data("large6_families.txt"), per_family=1, **{"lambda": 0.002}),
        "large6_multilambda_err": dict(tree=data("large6_tree.txt"), families=data("large6_families.txt"), per_family=1,
                                       lambdas="0.002,0.0035", lambda_tree=data("large6_lambda_tree.txt"), errfile=data("errormodel_900.txt")),
        "huge6_base": dict(tree=data("huge6_tree.txt"), families=data("huge6_families.txt"), per_family=1, **{"lambda": 0.0015}),
    }


def one_score(item):
    name, kv = item
    r = entry(kv, O.ref("score", **kv))
    print("ref score %s: -lnL %r M %d R %d" % (name, r["neg_lnl"], r["max_family_size"], r["max_root_family_size"]), flush=True)
    return name, r


def main():
    if not O.have_ref():
        raise SystemExit("oracle/_ref/ref_harness missing: run `make -C oracle ref` in the build container")
    write_tables()
    g = {"generator": "tests/golden/make_large_order_golden.py", "source": "oracle/_ref/ref_harness (real reference, g++ -O3 -fopenmp, no BLAS)"}
    # the longest jobs first: one thread per reference matrix, the scores' matrices spread over OpenMP threads
    with ThreadPoolExecutor(max_workers=6) as ex:
        mats = ex.map(one_matrix, sorted(matrix_pairs(), key=lambda j: -j[0]))
        scores = ex.map(one_score, sorted(score_jobs().items(), key=lambda kv: not kv[0].startswith("huge")))
        g["matrices"] = sorted(mats, key=lambda e: (e["n"], e["lambda"], e["t"]))
        g["scores"] = dict(sorted(scores))
    write_fixture(g)


if __name__ == "__main__":
    main()
