#!/usr/bin/env python3
"""Simulation (-s) at scale on the 100-taxon bench tree: cafe_simulate's device path, the driver's host path that follows
the reference draw for draw, and the driver end to end; plus one simulate-then-estimate round trip on mammals.

    python tools/simulate_scale.py OUT.json          (on the GPU box; profiles/simulate_scale.json keeps the record)

Device rows time capi.simulate (host planning, matrices, sampling, transposes and the copy back; root sizes and
multipliers are inputs), best of `reps` after a warm-up call.  Driver rows time whole cafexp_hip runs, whose JSON
separates the simulation from writing the two text files.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cafexp_amd import capi  # noqa: E402
from test_simulate import _tree  # noqa: E402

DATA = os.path.join(ROOT, "tests", "golden", "data")
EXE = os.path.join(ROOT, "cafexp_amd", "host", "cafexp_hip")
BENCH_TREE = os.path.join(DATA, "bench100_tree.txt")
# the compiled reference (g++ -O3, OpenMP, 8 threads) on the same tree, timed on a CPU host
REFERENCE = [
    {"command": "-l 0.002 -s2000", "families": 2000, "wall_s": 19.7, "cpu_s": 133.0},
    {"command": "-l 0.002 -k 4 -a 1.5 -s20000", "families": 20000, "wall_s": 191.5, "cpu_s": 1252.0},
]


def device_row(name, tree, F, alpha, node_sizes, reps=3, seed=1):
    rng = np.random.default_rng(seed)
    roots = rng.integers(0, 100, F).astype(np.int32)
    mult = rng.gamma(alpha, 1 / alpha, (F + 49) // 50) if alpha > 0 else None
    best = 1e30
    for _ in range(reps):
        t0 = time.perf_counter()
        leaf, nodes = capi.simulate(tree, [0.002], 100, roots, seed=seed, chunk_multiplier=mult, node_sizes=node_sizes)
        best = min(best, time.perf_counter() - t0)
    row = {"name": name, "families": F, "alpha": alpha, "node_sizes": node_sizes, "seconds": best, "families_per_s": F / best,
           "mean_leaf_size": float(leaf.mean())}
    print(json.dumps(row), flush=True)
    return row


def driver_row(name, args, timeout=900):
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        p = subprocess.run([EXE, "-t", BENCH_TREE, "-s", "7", "-o", tmp] + args, capture_output=True, text=True, timeout=timeout)
        wall = time.perf_counter() - t0
        assert p.returncode == 0, p.stderr
        info = json.loads(p.stdout.strip().splitlines()[-1])
        sizes = {f: os.path.getsize(os.path.join(tmp, f)) for f in ("simulation.txt", "simulation_truth.txt")}
    info.pop("multipliers", None)
    row = {"name": name, "args": " ".join(args), "wall_s": wall, "simulate_s": info["seconds"], "write_s": info["write_seconds"],
           "families": info["n_families"], "families_per_s": info["n_families"] / info["seconds"], "mode": info["mode"], "bytes": sizes}
    print(json.dumps(row), flush=True)
    return row


def round_trip():
    tree = os.path.join(DATA, "mammals_tree.txt")
    with tempfile.TemporaryDirectory() as tmp:
        p = subprocess.run([EXE, "-t", tree, "-l", "0.01", "--simulate", "20000", "--simulate-device", "-s", "3", "-o", tmp],
                           capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr
        e = subprocess.run([EXE, "-t", tree, "-i", os.path.join(tmp, "simulation.txt")], capture_output=True, text=True, timeout=600)
        assert e.returncode == 0, e.stderr
        info = json.loads(e.stdout.strip().splitlines()[-1])
    lam = info["lambda"][0]
    row = {"name": "round trip mammals lambda 0.01, 20000 device families", "lambda_hat": lam, "relative_error": abs(lam - 0.01) / 0.01,
           "families_estimated": info["n_families"]}
    print(json.dumps(row), flush=True)
    return row


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else "simulate_scale.json"
    tree = _tree("bench100_tree.txt")
    capi.simulate(tree, [0.002], 100, np.ones(1000, dtype=np.int32), seed=1)          # HIP start-up
    rows = [
        device_row("device base 1M, leaves + all nodes", tree, 1_000_000, 0.0, True),
        device_row("device base 1M, leaves only", tree, 1_000_000, 0.0, False),
        device_row("device gamma alpha 1.5 1M, leaves + all nodes", tree, 1_000_000, 1.5, True),
        device_row("device gamma alpha 1.5 1M, leaves only", tree, 1_000_000, 1.5, False),
        driver_row("driver host path base 20k", ["-l", "0.002", "--simulate", "20000"]),
        driver_row("driver host path gamma k 4 alpha 1.5 20k", ["-l", "0.002", "-k", "4", "-a", "1.5", "--simulate", "20000"]),
        driver_row("driver device path base 20k", ["-l", "0.002", "--simulate", "20000", "--simulate-device"]),
        driver_row("driver device path base 1M (both files)", ["-l", "0.002", "--simulate", "1000000", "--simulate-device"]),
        driver_row("driver device path gamma alpha 1.5 1M (both files)", ["-l", "0.002", "-a", "1.5", "--simulate", "1000000", "--simulate-device"]),
        round_trip(),
    ]
    with open(out, "w") as f:
        json.dump({"tree": "tests/golden/data/bench100_tree.txt", "rows": rows, "reference": REFERENCE}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
