#!/usr/bin/env python3
"""Lambda-per-family mode (-b) at scale: one cafe_score_per_family evaluation over a whole table, and the whole -b run on
the mammals table.

    python tools/lambda_per_family_scale.py OUT.json     (on the GPU box; profiles/lambda_per_family_scale.json keeps the record)

Evaluation rows: every family of the table gets its own lambda (spread around the table's global estimate), best of `reps`
calls after a warm-up; a row step is one step of the row recurrence of one (family, branch) wave, so an evaluation runs
families x branches x rows of them.  The roof they are judged against is K1's store-less build (tools/k1_time.py with
-D'CAFE_EXPERIMENT_K1_STORE_IF=&& n < 0', DESIGN.md section 3: 1320 matrices of order 751, 0.69 ms for the chain of row
steps): the fused kernel is that chain plus a dot product.  The driver row times `cafexp_hip -b` end to end.  The reference
rate is quoted from tests/golden/ref_lambda_per_family.json: another machine (a CPU build container), labelled so.
"""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cafexp_amd import capi, problem as P, synth  # noqa: E402

DATA = os.path.join(ROOT, "tests", "golden", "data")
EXE = os.path.join(ROOT, "cafexp_amd", "host", "cafexp_hip")
K1_STORELESS = {"matrices": 1320, "order": 751, "ms": 0.69, "source": "DESIGN.md section 3 (tools/k1_time.py, store-less build)"}


def read(name):
    with open(os.path.join(DATA, name)) as f:
        return f.read()


def evaluation_row(name, pb, lam_mid, reps=3):
    prior = P.prior_uniform(pb.max_root_family_size)
    pr = P.Params(lambdas=np.array([lam_mid]), prior=prior)
    rng = np.random.default_rng(1)
    lam = lam_mid * (0.5 + rng.random(pb.n_families))
    fam = np.arange(pb.n_families)
    ctx = capi.Context(pb)
    try:
        got = ctx.score_per_family(pr, fam, lam)
        best = 1e30
        for _ in range(reps):
            t0 = time.perf_counter()
            ctx.score_per_family(pr, fam, lam)
            best = min(best, time.perf_counter() - t0)
        t0 = time.perf_counter()
        ctx.score(pr)
        ctx.score(pr)
        shared_ms = (time.perf_counter() - t0) / 2 * 1e3
    finally:
        ctx.close()
    is_root_child = np.asarray(pb.parent) == int(np.argmax(np.asarray(pb.parent) < 0))
    rows = int(np.sum(np.where(is_root_child, pb.max_root_family_size + 1, pb.max_family_size + 1)[np.asarray(pb.parent) >= 0]))
    steps = pb.n_families * rows
    roof = K1_STORELESS["matrices"] * K1_STORELESS["order"] / (K1_STORELESS["ms"] * 1e-3)
    row = {"name": name, "families": pb.n_families, "branches": pb.n_nodes - 1, "matrix_order": pb.matrix_size, "ms": best * 1e3,
           "row_steps": steps, "row_steps_per_s": steps / best, "finite": int(np.isfinite(got).sum()),
           "one_shared_lambda_scorer_call_ms": shared_ms}
    if pb.matrix_size == K1_STORELESS["order"]:
        row["k1_storeless_row_steps_per_s"] = roof
        row["time_per_matrix_over_k1_storeless"] = roof / row["row_steps_per_s"]
    print(json.dumps(row), flush=True)
    return row


def driver_row(timeout=1500):
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        p = subprocess.run([EXE, "-t", os.path.join(DATA, "mammals_tree.txt"), "-i", os.path.join(DATA, "mammal_gene_families.txt"), "-b", "-s", "7",
                            "-o", tmp], capture_output=True, text=True, timeout=timeout)
        wall = time.perf_counter() - t0
        assert p.returncode == 0, p.stderr
        info = json.loads(p.stdout.strip().splitlines()[-1])
        lines = open(os.path.join(tmp, "Base_lambda_per_family.txt")).read().count("\n")
    row = {"name": "cafexp_hip -b, mammal_gene_families.txt", "wall_s": wall, "search_s": info["seconds"], "families": info["families"],
           "distinct_families": info["distinct_families"], "rounds": info["rounds"], "evaluations": info["evaluations"], "lines": lines}
    print(json.dumps(row), flush=True)
    return row


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else "lambda_per_family_scale.json"
    species, ids, counts = P.read_family_table(read("mammal_gene_families.txt"))
    mammals = P.build_problem(P.parse_newick(read("mammals_tree.txt")), species, ids, counts)
    bench, _ = synth.make_problem(n_taxa=100, n_families=2000, max_count=600)
    rows = [evaluation_row("one evaluation, mammal_gene_families.txt", mammals, 0.005),
            evaluation_row("one evaluation, bench table (100 taxa, order 751), 2000 families", bench, 0.002),
            driver_row()]
    with open(os.path.join(ROOT, "tests", "golden", "ref_lambda_per_family.json")) as f:
        fx = json.load(f)["cases"]
    reference = [{"case": k, "families": v["n_families"], "seconds": v["seconds"], "threads": v["threads"],
                  "seconds_per_family": v["seconds"] / v["n_families"],
                  "machine": "CPU build container, not the GPU host; run next to a compile job"} for k, v in sorted(fx.items())]
    with open(out, "w") as f:
        json.dump({"rows": rows, "k1_storeless": K1_STORELESS, "reference": reference}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
