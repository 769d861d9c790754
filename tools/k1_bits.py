"""Scratch: the bits of K1 and of the per-family kernel, for comparing two builds of the library -- sibling of tools/k1_time.py.

    python tools/k1_bits.py [--lib PATH/libcafe_mi355x.so] > OUT.txt        (on a machine with the GPU)

One SHA-256 per (matrix order, layout, rate model) of what cafe_build_matrices / cafe_build_matrices_lm return: one order per
width E = 2 .. 32 of the kernels in both layouts, two live keys and a saturated one, the two-rate entry at mu = lambda,
0.7 lambda and 1.7 lambda.  Then one per (order, rate model) of the values of cafe_score_per_family / cafe_score_per_family_lm
on the three-taxon table of tests/test_per_family_shapes.py.  Two builds compute the same when the two outputs are equal."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cafexp_amd import capi, problem as P  # noqa: E402

if len(sys.argv) > 2 and sys.argv[1] == "--lib":
    capi.LIB_PATH = os.path.abspath(sys.argv[2])
capi.load()

ORDERS = [2, 128, 129, 257, 385, 513, 641, 769, 897, 1025, 1281, 1537, 1793, 2048]
LAM, T = np.array([0.006335, 0.01, 0.05]), np.array([68.7105, 30.0, 40.0])          # the third key is saturated at mu = lambda
MODELS = (("lambda = mu", None), ("mu = lambda", 1.0), ("mu = 0.7 lambda", 0.7), ("mu = 1.7 lambda", 1.7))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


for n in ORDERS:
    for layout in (0, 1):
        for label, ratio in MODELS:
            m = capi.build_matrices(n, LAM, T, layout=layout) if ratio is None else capi.build_matrices_lm(n, LAM, ratio * LAM, T, layout=layout)
            print("matrices order %4d layout %d %-16s %s" % (n, layout, label, sha(m)), flush=True)

from helpers import _explicit_problem  # noqa: E402
from test_per_family_shapes import LAMBDAS, TREE3, families, sizes  # noqa: E402

lam = np.array(LAMBDAS)
for n in ORDERS[1:]:
    M, R = sizes(n)
    pb = _explicit_problem(TREE3, families(n), M, R)
    pr = P.Params(lambdas=np.ones(1), prior=P.prior_uniform(R))
    ctx = capi.Context(pb)
    for label, ratio in MODELS:
        v = ctx.score_per_family(pr, np.arange(4), lam) if ratio is None else ctx.score_per_family_lm(pr, np.arange(4), lam, ratio * lam)
        print("per-family order %4d %-16s %s" % (n, label, sha(v)), flush=True)
    ctx.close()
