#!/usr/bin/env python3
"""Generates tests/golden/ref_simulate.json from the REAL reference's simulator (-s).

Run in the build container only (needs the reference and `make -C oracle ref`):
    python tests/golden/make_simulate_golden.py
Every case runs `oracle/_ref/ref_harness cafexp <args> -o DIR`, i.e. the reference program's own main at the harness's
fixed engine seed 10, and records the text of DIR/simulation.txt and DIR/simulation_truth.txt, the "Average multiplier"
line when there is one, and the exit code (with the message of a failing run).  Paths in `args` are relative to
tests/golden/data.  The fixture holds outputs only; no reference source is stored.
"""
import json
import os
import re
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
D = os.path.join(HERE, "data")
HARNESS = os.path.join(ROOT, "oracle", "_ref", "ref_harness")

# name -> reference arguments (file names relative to tests/golden/data)
CASES = {
    "base": ["-t", "mammals_tree.txt", "-l", "0.01", "-s200"],
    "gamma": ["-t", "mammals_tree.txt", "-k", "3", "-a", "0.5", "-l", "0.01", "-s260"],
    "rootdist_pared": ["-t", "mammals_tree.txt", "-l", "0.01", "-f", "poisson_root_dist_1000.txt", "-s40"],
    "rootdist_full": ["-t", "mammals_tree.txt", "-l", "0.01", "-f", "rootdist_small.txt", "-s"],
    "error_model": ["-t", "mammals_tree.txt", "-l", "0.01", "-e", "errormodel_600.txt", "-s60"],
    "multi_lambda": ["-t", "mammals_tree.txt", "-m", "0.01,0.05", "-y", "chimphuman_separate_lambda.txt", "-s60"],
    "error_model_too_small": ["-t", "mammals_tree.txt", "-l", "0.01", "-e", "errormodel_0.1.txt", "-s30"],
}
DATA_FLAGS = {"-t", "-f", "-y"}


def ref_args(args):
    """Data paths made absolute; -e FILE becomes -eFILE (the reference's -e takes an optional, glued argument)."""
    out = []
    for i, a in enumerate(args):
        if a == "-e":
            continue
        if i > 0 and args[i - 1] == "-e":
            out.append("-e" + os.path.join(D, a))
        elif i > 0 and args[i - 1] in DATA_FLAGS:
            out.append(os.path.join(D, a))
        else:
            out.append(a)
    return out


def run(args):
    with tempfile.TemporaryDirectory() as tmp:
        out_dir = os.path.join(tmp, "out")
        p = subprocess.run([HARNESS, "cafexp"] + ref_args(args) + ["-o", out_dir], capture_output=True, text=True, timeout=600, cwd=tmp)
        m = re.search(r"^Average multiplier for simulated values: (.*)$", p.stdout, re.M)
        rec = {"args": args, "rc": p.returncode, "average_multiplier": m.group(1) if m else None}
        if p.returncode == 0:
            for name in ("simulation.txt", "simulation_truth.txt"):
                with open(os.path.join(out_dir, name)) as f:
                    rec[name] = f.read()
        else:
            rec["message"] = [l for l in p.stdout.splitlines() if l.strip() and not l.startswith(("{", "Filtering", "Simulating"))][-1]
        return rec


def main():
    cases = {name: run(args) for name, args in CASES.items()}
    path = os.path.join(HERE, "ref_simulate.json")
    with open(path, "w") as f:
        json.dump({"seed": 10, "cases": cases}, f, indent=0, sort_keys=True)
        f.write("\n")
    for name, c in cases.items():
        rows = c.get("simulation.txt", "").count("\n") - 1
        print("%-22s rc %d rows %4d avg %s %s" % (name, c["rc"], rows, c["average_multiplier"], c.get("message", "")))
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
