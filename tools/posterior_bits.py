"""Scratch: the bits of the three posterior calls, for comparing two builds of the library -- sibling of tools/k1_bits.py.

    python tools/posterior_bits.py [--lib PATH/libcafe_mi355x.so] > OUT.txt        (on a machine with the GPU)

One SHA-256 per output array of cafe_marginal_reconstruct, cafe_sample_histories (fixed seed; sizes, counts and categories)
and cafe_score_gradient (both root rules; lambda = mu and death rates set) on tests/test_marginal_shapes.py's sweep_case at
five (M, R) pairs, base model and gamma K = 2 with a 3-tap error model.  Then one case per call whose workspace limit forces
three or more column batches, sized as the tests' batch cases size theirs.  Two builds compute the same when the two outputs
are equal."""
import dataclasses
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cafexp_amd import capi, problem as P  # noqa: E402
from cafexp_amd.gamma_rates import discrete_gamma  # noqa: E402

if len(sys.argv) > 2 and sys.argv[1] == "--lib":
    capi.LIB_PATH = os.path.abspath(sys.argv[2])
capi.load()

import history_ref as HR  # noqa: E402
import test_gradient_shapes as GS  # noqa: E402
import test_marginal_shapes as MS  # noqa: E402
from test_per_family_shapes import THREE_TAPS  # noqa: E402

PAIRS = [(2, 2), (63, 64), (65, 129), (126, 62), (257, 385)]
DRAWS, SEED = 5, (751 << 32) + 0x5EED
kBN = 128


def show(label, res):
    for key in sorted(res):
        print("%-58s %-14s %s" % (label, key, hashlib.sha256(np.ascontiguousarray(res[key]).tobytes()).hexdigest()), flush=True)


def K_of(pr):
    return 1 if pr.multipliers is None else len(pr.multipliers)


def three_calls(label, pb, pr, alpha):
    ctx = capi.Context(pb, max_categories=K_of(pr))
    show(label + " marginal", ctx.marginal_reconstruct(pr, alpha=alpha))
    show(label + " history", ctx.sample_histories(pr, DRAWS, SEED, alpha=alpha))
    for mus in (None, 0.8 * pr.lambdas):
        ctx.set_death_rates(mus)
        for rule in ("max", "sum"):
            show("%s gradient %s %s" % (label, rule, "lambda = mu" if mus is None else "mu = 0.8 lambda"), ctx.score_gradient(pr, rule, alpha=alpha))
    ctx.close()


for M, R in PAIRS:
    pb, pr = MS.sweep_case(M, R)
    three_calls("M %3d R %3d base" % (M, R), pb, pr, 1.0)
    gpr = dataclasses.replace(pr, error_model=P.error_model_table(THREE_TAPS, M))
    gpr.cat_probs, gpr.multipliers = discrete_gamma(2, 0.7)
    three_calls("M %3d R %3d gamma 2, 3 taps" % (M, R), dataclasses.replace(pb, n_deviations=3), gpr, 0.7)

# ---- three column batches, marginal: the problem of test_a_partial_last_batch_changes_no_bit, 128 columns per batch of 384
rng = np.random.default_rng(62)
tree = P.parse_newick(MS.SWEEP_TREE)
names = [leaf.name for leaf in tree.leaves()]
counts = rng.integers(0, 15, size=(300, len(names))).astype(np.int32)
counts[0], counts[1], counts[2] = 0, 129, 128
pb = P.build_problem(tree, names, ["f%d" % i for i in range(300)], counts, root_filter=False, n_deviations=3, max_family_size=129, max_root_family_size=100)
pr = P.Params(lambdas=np.array([0.02]), prior=P.prior_uniform(100), error_model=P.error_model_table(THREE_TAPS, 129))
pr.cat_probs, pr.multipliers = discrete_gamma(3, 0.5)
per_col = MS._per_col(pb, 3)
ctx = capi.Context(pb, max_categories=3, workspace_limit=kBN * per_col + per_col // 2)
assert -(-ctx.stats()["n_unique_families"] // kBN) == 3
show("three batches marginal", ctx.marginal_reconstruct(pr, alpha=0.5))
ctx.close()

# ---- gradient: the problem of test_three_column_batches_change_no_bit
cfg = GS.CONFIGS["gamma_err_rho_0.25"]
pb = GS._problem(40, 30, n=300, seed=300, err=True, distinct=True)
pr = GS._params(pb, cfg)
per_col = GS._per_col(pb, 3, 2)
ctx = capi.Context(pb, max_categories=3, workspace_limit=kBN * per_col + per_col // 2)
assert -(-ctx.stats()["n_unique_families"] // kBN) == 3
ctx.set_death_rates(cfg["mus"])
show("three batches gradient", ctx.score_gradient(pr, "max", alpha=0.7))
ctx.close()

# ---- history: the problem and the limit of test_same_bits_twice_in_batches_and_across_duplicates
case = HR._case(HR.CATERPILLAR, 24, 20, 90, 100, 33, 22, gamma=3)
pb = case["pb"]
reps = np.repeat(np.arange(pb.n_families), 4)
big = dataclasses.replace(pb, counts=np.ascontiguousarray(pb.counts[reps]), family_ids=["d%d" % i for i in range(len(reps))])
nI = int((pb.leaf_taxon < 0).sum())
per_col = (2 * nI * pb.matrix_size + case["K"] + 1) * 8
ctx = capi.Context(big, max_categories=case["K"], dedup=False, workspace_limit=(190 * per_col * 4) // 3 + 3 * case["n_draws"] * pb.n_nodes * 8)
got = ctx.sample_histories(case["pr"], case["n_draws"], case["seed"], alpha=case["alpha"])
batches, passes = ctx.history_batches()
assert batches >= 3 and passes > 1, (batches, passes)
show("%d batches, %d passes history" % (batches, passes), got)
ctx.close()
