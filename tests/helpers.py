"""Shared test plumbing: rebuild a (Problem, Params) pair from a golden fixture's argument record; the compiler's resource
remarks of one HIP file."""
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from cafexp_amd import problem as P

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cafexp_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@functools.lru_cache(maxsize=None)
def kernel_resources(hip_file):
    """Cross-compiles cafexp_amd/csrc/<hip_file> for gfx950 with the Makefile's FLAGS (CPU only, device code only) and returns
    the compiler's resource remarks as {mangled kernel name: {remark: value}} -- what `make check` reads.  Skips without hipcc."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    with open(os.path.join(CSRC, "Makefile")) as f:
        flags = next(ln for ln in f if ln.startswith("FLAGS")).split(":=", 1)[1].replace("$(ARCH)", "gfx950").split()
    r = subprocess.run([HIPCC] + flags + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", hip_file, "-o", os.devnull],
                       cwd=CSRC, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[a-zA-Z/]+\])?: (\d+)", line)
        if m and name:
            kernels[name][m.group(1).strip()] = int(m.group(2))
    return kernels


def read(name):
    with open(os.path.join(DATA, name)) as f:
        return f.read()


_cache = {}


def table(name):
    if name not in _cache:
        _cache[name] = P.read_family_table(read(name))
    return _cache[name]


def case_from_args(args, oracle):
    """args: the `args` dict of a tests/golden/ref_golden.json score entry (ref_harness job_score keys)."""
    tree = P.parse_newick(read(args["tree"]))
    species, ids, counts = table(args["families"])
    lam_tree = P.parse_newick(read(args["lambda_tree"]), lambda_tree=True) if "lambda_tree" in args else None
    n_dev, dists = 0, None
    if "errfile" in args:
        _, dev, dists = P.read_error_model(read(args["errfile"]))
        n_dev = len(dev)
    pb = P.build_problem(tree, species, ids, counts, lambda_tree=lam_tree, root_filter=bool(int(args.get("rootfilter", 1))),
                         n_deviations=n_dev)
    if "limit" in args:
        lim = int(args["limit"])
        pb.counts = np.ascontiguousarray(pb.counts[:lim])
        pb.family_ids = pb.family_ids[:lim]
    if "lambdas" in args:
        lambdas = np.array([float(x) for x in str(args["lambdas"]).split(",")])
    else:
        lambdas = np.array([float(args["lambda"])])
    R = pb.max_root_family_size
    prior_spec = args.get("prior", "uniform")
    if "rootdist" in args:
        rd = {}
        for line in read(args["rootdist"]).splitlines():
            tk = line.split()
            if len(tk) >= 2:
                rd[int(tk[0])] = int(tk[1])
        prior = P.prior_rootdist(R, rd)
    elif prior_spec == "uniform":
        prior = P.prior_uniform(R)
    else:
        prior = P.prior_poisson(R, float(prior_spec.split(":")[1]))
    pr = P.Params(lambdas=lambdas, prior=prior)
    alpha = 1.0
    if args.get("model", "base") == "gamma":
        alpha = float(args["alpha"])
        probs, mult = oracle.discrete_gamma(int(args["k"]), alpha)
        pr.multipliers, pr.cat_probs = mult, probs
    if dists is not None:
        pr.error_model = P.error_model_table(dists, pb.max_family_size)
    return pb, pr, alpha


def _explicit_problem(newick, rows, M, R):
    """rows: one {species: count} dict per family.  M and R are given: pb.matrix_size == max(M, R) + 1."""
    tree = P.parse_newick(newick)
    species = sorted(rows[0])
    table = np.array([[r[s] for s in species] for r in rows], dtype=np.int32)
    return P.build_problem(tree, species, ["f%d" % i for i in range(len(rows))], table, root_filter=False,
                           max_family_size=M, max_root_family_size=R)


def rel_err(a, b):
    if np.isinf(a) or np.isinf(b):
        return 0.0 if a == b else np.inf
    return abs(a - b) / max(abs(b), 1e-300)
