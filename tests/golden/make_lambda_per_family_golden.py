#!/usr/bin/env python3
"""Generates tests/golden/ref_lambda_per_family.json from the REAL reference's lambda-per-family mode (-b).

Run in the build container only (needs the reference and `make -C oracle ref`):
    python tests/golden/make_lambda_per_family_golden.py [case ...]
Every case runs `oracle/_ref/ref_harness cafexp <args> -b -o DIR`, i.e. the reference program's own main at the
harness's fixed engine seed 10, and records the text of DIR/Base_lambda_per_family.txt, the wall seconds and the
thread count.  Paths in `args` are relative to tests/golden/data.  Without case names every case is run; with names,
only those are run and the others are kept from the existing fixture.  The fixture holds outputs only; no reference
source is stored.  The reference needs about 6 s per family (one lambda) and 20 s per family (two) on 8 threads.
"""
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
D = os.path.join(HERE, "data")
HARNESS = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
SOURCE_TABLE = "mammal_gene_families.txt"

# name -> (families taken from the head of the mammals table, reference arguments without -i / -b)
CASES = {
    "mammals24": (24, ["-t", "mammals_tree.txt"]),
    "mammals8_poisson": (8, ["-t", "mammals_tree.txt", "-p"]),
    "mammals6_lambda_tree": (6, ["-t", "mammals_tree.txt", "-y", "chimphuman_separate_lambda.txt"]),
    "mammals6_errormodel": (6, ["-t", "mammals_tree.txt", "-e", "errormodel_600.txt"]),
}
DATA_FLAGS = {"-t", "-y"}


def head_table(n):
    with open(os.path.join(D, SOURCE_TABLE)) as f:
        lines = f.readlines()
    return "".join(lines[:n + 1])


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


def run(n_families, args):
    threads = int(os.environ.get("OMP_NUM_THREADS", "8"))
    env = dict(os.environ, OMP_NUM_THREADS=str(threads))
    with tempfile.TemporaryDirectory() as tmp:
        table = os.path.join(tmp, "families.txt")
        with open(table, "w") as f:
            f.write(head_table(n_families))
        out_dir = os.path.join(tmp, "out")
        t0 = time.time()
        p = subprocess.run([HARNESS, "cafexp"] + ref_args(args) + ["-i", table, "-b", "-o", out_dir], capture_output=True, text=True,
                           timeout=3000, cwd=tmp, env=env)
        seconds = time.time() - t0
        if p.returncode != 0:
            raise SystemExit("reference failed (%d): %s" % (p.returncode, p.stdout[-2000:] + p.stderr[-2000:]))
        with open(os.path.join(out_dir, "Base_lambda_per_family.txt")) as f:
            text = f.read()
    return {"args": args, "n_families": n_families, "table_head_of": SOURCE_TABLE, "Base_lambda_per_family.txt": text,
            "seconds": round(seconds, 1), "threads": threads}


def main():
    path = os.path.join(HERE, "ref_lambda_per_family.json")
    cases = {}
    if os.path.exists(path):
        with open(path) as f:
            cases = json.load(f)["cases"]
    with open(os.path.join(D, "mammals_24.txt"), "w") as f:
        f.write(head_table(24))
    for name in (sys.argv[1:] or list(CASES)):
        cases[name] = run(*CASES[name])
        c = cases[name]
        print("%-22s %3d families %3d lines %7.1f s on %d threads" % (name, c["n_families"], c["Base_lambda_per_family.txt"].count("\n"),
                                                                     c["seconds"], c["threads"]), flush=True)
        with open(path, "w") as f:
            json.dump({"seed": 10, "cases": cases}, f, indent=0, sort_keys=True)
            f.write("\n")
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
