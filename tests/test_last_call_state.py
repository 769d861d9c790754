"""What a context's read-backs accept after each kind of call, and which captured graph a call replays.

The context remembers one thing about its last call (cafe_ctx::last, cafe_ctx.h): none / rejected / scored / matrices only.
The first test walks one context through every way into each of these and pins, per step, which read-backs raise and which
return; the table was taken from the library before the four states had a name.  The second interleaves every mode that has
a graph of its own on a graph-replaying context and a stream-path one: a call that found another mode's graph under its
key would return that mode's value."""
import math

import numpy as np
import pytest

from cafexp_amd import problem as P, synth
from cafexp_amd.gamma_rates import discrete_gamma

pytestmark = pytest.mark.gpu

READERS = ("family_results", "matrix", "root_likelihoods", "extents", "k_ranges", "executed_flops")
NONE = ()
MATRICES_ONLY = tuple(r for r in READERS if r != "family_results")


@pytest.fixture(scope="module")
def capi():
    from cafexp_amd import capi as C
    C.load()
    return C


def _case(max_count):
    pb, _ = synth.make_problem(n_taxa=14, n_families=900, max_count=max_count, lam_sim=0.004, seed=9, root_cap=35)
    return pb, P.Params(lambdas=np.array([0.004]), prior=P.prior_uniform(pb.max_root_family_size))


@pytest.fixture(scope="module")
def case():
    return _case(50)


def _gamma(pr, K, alpha):
    probs, mult = discrete_gamma(K, alpha)
    return P.Params(lambdas=pr.lambdas, prior=pr.prior, multipliers=mult, cat_probs=probs)


def _accepted(capi, ctx, node):
    calls = {"family_results": lambda: ctx.family_results(0), "matrix": lambda: ctx.matrix(node), "root_likelihoods": lambda: ctx.root_likelihoods(0),
             "extents": lambda: ctx.extents(node), "k_ranges": lambda: ctx.k_ranges(node), "executed_flops": ctx.executed_flops}
    ok = []
    for name in READERS:
        try:
            calls[name]()
            ok.append(name)
        except capi.CafeError:
            pass
    return tuple(ok)


# Matrices below order 256 publish no extents (cafe_create.hip): there cafe_get_extents and cafe_debug_k_ranges refuse whatever
# the state, so the second shape is the one that shows the state through them.
@pytest.mark.parametrize("max_count,switched_off", [(50, ("extents", "k_ranges")), (230, ())], ids=["order<256", "order>=256"])
def test_which_read_backs_each_kind_of_call_leaves_open(capi, max_count, switched_off):
    pb, pr = _case(max_count)
    assert (pb.max_family_size + 1 >= 256) == (not switched_off)
    node = next(v for v in range(pb.n_nodes) if pb.leaf_taxon[v] < 0 and pb.parent[v] >= 0)     # interior, not the root: has a K2 op
    ctx = capi.Context(pb)
    seen = {}

    def step(name):
        seen[name] = _accepted(capi, ctx, node)

    step("fresh")
    assert ctx.score(P.Params(lambdas=np.array([0.0]), prior=pr.prior)) == math.inf       # rejected on the host (lambda.h:58)
    step("rejected")
    want = ctx.score(pr)
    assert math.isfinite(want)
    step("scored")
    ctx.root_max(pr.lambdas)
    step("root_max")
    ctx.marginal_reconstruct(pr)
    step("marginal_reconstruct")
    ctx.score_per_family(pr, [0, 1, 2], [0.004, 0.005, 0.006])
    step("score_per_family")
    ctx.debug_fail_next(1)
    with pytest.raises(capi.CafeError, match="injected failure"):
        ctx.score(pr)
    step("failed")
    assert ctx.score(pr) == want
    step("scored again")
    ctx.close()
    for name, got in seen.items():
        print(name, got)
    want = {"fresh": NONE, "rejected": NONE, "scored": READERS, "root_max": MATRICES_ONLY, "marginal_reconstruct": MATRICES_ONLY,
            "score_per_family": NONE, "failed": NONE, "scored again": READERS}
    assert seen == {name: tuple(r for r in ok if r not in switched_off) for name, ok in want.items()}


def test_every_mode_replays_its_own_graph(capi, case):
    pb, pr = case
    g2, g3 = _gamma(pr, 2, 1.5), _gamma(pr, 3, 0.8)
    stream, graphs = capi.Context(pb, max_categories=3), capi.Context(pb, max_categories=3)
    graphs.set_graphs(True)

    def score(p, alpha):
        def run(ctx):
            v, fam = ctx.score(p, alpha=alpha, per_family=True)
            return np.concatenate([[v], fam["family_lnl"]])
        return run

    def both(setter):
        for ctx in (stream, graphs):
            setter(ctx)

    def round_of_calls():
        out = []
        for run in (score(pr, 1.0), score(g2, 1.5), score(g3, 0.8)):
            out.append([run(ctx) for ctx in (stream, graphs)])
        both(lambda ctx: ctx.set_root_rule("sum"))
        for run in (score(pr, 1.0), score(g2, 1.5), score(g3, 0.8)):
            out.append([run(ctx) for ctx in (stream, graphs)])
        both(lambda ctx: ctx.set_root_rule("max"))
        both(lambda ctx: ctx.set_death_rates([0.003]))
        out.append([score(pr, 1.0)(ctx) for ctx in (stream, graphs)])
        out.append([ctx.root_max(pr.lambdas) for ctx in (stream, graphs)])
        both(lambda ctx: ctx.set_death_rates(None))
        out.append([ctx.root_max(pr.lambdas) for ctx in (stream, graphs)])
        return out

    rounds = [round_of_calls(), round_of_calls()]             # the first captures, the second only replays
    stream.close()
    graphs.close()
    for r in rounds:
        for i, (a, b) in enumerate(r):
            assert np.array_equal(a, b, equal_nan=True), "call %d: the graph replay differs from the stream path" % i
    for a, b in zip(*rounds):
        assert np.array_equal(a[0], b[0], equal_nan=True)
    firsts = [r[0][0] for r in rounds[0][:7]]                  # the seven scorer modes do differ: a wrong graph would show
    assert len({float(v) for v in firsts}) == 7
