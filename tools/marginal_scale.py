"""Marginal reconstruction at scale: wall time of cafe_marginal_reconstruct on the mammals table and on the bench table
(50 000 families, 100 taxa, N = 751, K = 1), cafe_reconstruct at the same shapes, and the achieved fp64 rate of the GEMM
kernel (HIP events around its launches) against the 78.6 TFLOP/s MFMA peak.  One process, one GPU; writes
profiles/marginal_scale.json."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from cafexp_amd import capi, problem as P, synth

PEAK_TFLOPS = 78.6


def measure(name, pb, lam):
    pr = P.Params(lambdas=np.array([lam]), prior=P.prior_uniform(pb.max_root_family_size))
    jmax = min(pb.max_family_size, pb.max_root_family_size)
    rp = np.zeros(jmax + 1, dtype=np.float32)
    rp[:pb.max_root_family_size] = P.prior_uniform(pb.max_root_family_size)[:jmax + 1]
    ctx = capi.Context(pb)
    ctx.score(pr)
    rec = {"table": name, "families": pb.n_families, "unique_families": int(ctx.stats()["n_unique_families"]), "nodes": pb.n_nodes,
           "matrix_order": pb.matrix_size, "K": 1}
    walls = []
    for _ in range(3):
        t = time.perf_counter()
        res = ctx.marginal_reconstruct(pr)
        walls.append(time.perf_counter() - t)
    rec["marginal_seconds"] = walls
    rec["marginal_failed"] = int(res["failed"].sum())
    ctx.set_profiling(True)
    t = time.perf_counter()
    ctx.marginal_reconstruct(pr)
    rec["marginal_seconds_profiled"] = time.perf_counter() - t
    ms, flops = ctx.marginal_gemm_stats()
    ctx.set_profiling(False)
    rec["gemm_ms"], rec["gemm_flops"] = ms, flops
    rec["gemm_tflops"] = flops / (ms * 1e-3) / 1e12 if ms > 0 else None
    rec["gemm_fraction_of_peak"] = rec["gemm_tflops"] / PEAK_TFLOPS if ms > 0 else None
    walls = []
    for _ in range(3):
        t = time.perf_counter()
        ctx.reconstruct(pr.lambdas, rp)
        walls.append(time.perf_counter() - t)
    rec["joint_reconstruct_seconds"] = walls
    ctx.close()
    print(json.dumps(rec), flush=True)
    return rec


def main():
    F = int(sys.argv[1]) if len(sys.argv) > 1 else 50000
    data = os.path.join(ROOT, "tests", "golden", "data")
    with open(os.path.join(data, "mammal_gene_families.txt")) as f:
        species, ids, counts = P.read_family_table(f.read())
    with open(os.path.join(data, "mammals_tree.txt")) as f:
        mammals = P.build_problem(P.parse_newick(f.read()), species, ids, counts)
    bench, _ = synth.make_problem(n_families=F)
    out = {"peak_tflops": PEAK_TFLOPS, "runs": [measure("mammals", mammals, 0.0018), measure("bench", bench, 0.002)]}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "marginal_scale.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
