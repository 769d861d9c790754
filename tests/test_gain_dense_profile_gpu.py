"""The slot layouts of the four profile entries of the gain dense path (cafe_debug_gain_dense, _dense_posterior, _predictive and
_marginal): every entry publishes the launches of its own call's last run and of no other call's.  One context, profiling on, the
four calls in turn on a three-entry list of the first case of tests/gain_marginal_ref.py (a caterpillar: interior nodes and leaves
at every depth, so every kind of kernel a call has is launched)."""
from contextlib import closing

import numpy as np
import pytest

import gain_marginal_ref as GM
from test_gain_posterior_gpu import capi  # noqa: F401 (the fixture)

RATES = [[r] for r in GM.RATES]
# (the call, its profile entry, published slots, the slots whose kernel kind the call launches)
ENTRIES = (("score_gain", "gain_dense_profile", 4, range(4)),                     # build, product, GEMM, root
           ("gain_posterior_dense", "gain_dense_posterior_profile", 8, range(8)),  # + weights, transposed GEMM, interior and leaf outputs
           ("gain_leaf_predictive", "gain_predictive_profile", 7, range(7)),       # + weights, transposed GEMM, the fused leaf kernel
           ("gain_marginal_dense", "gain_marginal_profile", 9, range(9)))          # the posterior's eight with its own kernels, their total


def _call(ctx, pr, name, fam):
    args = (pr, fam) + tuple(RATES) + (GM.ABSENT,)
    return getattr(ctx, name)(*(args + (GM.LEVEL,) if name == "gain_marginal_dense" else args))


def _profiles(ctx):
    return {entry: getattr(ctx, entry)() for _, entry, _, _ in ENTRIES}


@pytest.mark.gpu
def test_every_profile_entry_publishes_its_own_call_in_its_own_slots(capi):
    pb, pr = GM.problem(*GM.CASES[0])
    fam = np.array([0, 3, capi.CAFE_FAMILY_ABSENT])
    with closing(capi.Context(pb)) as ctx:
        ctx.set_profiling(True)
        for name, entry, slots, launched in ENTRIES:
            before = _profiles(ctx)
            _call(ctx, pr, name, fam)
            after = _profiles(ctx)
            ms, flops = after[entry]
            print(name, list(ms), flops)
            assert ms.shape == (slots,) and np.isfinite(ms).all() and (ms >= 0).all(), (name, ms)
            assert all(ms[k] > 0 for k in launched) and flops > 0, (name, ms, flops)
            if name == "gain_leaf_predictive":
                assert ms[6] > 0
            if name == "gain_marginal_dense":
                total = 0.0
                for k in range(8):
                    total += ms[k]
                assert ms[8] == total
            for other in before:
                if other != entry:
                    assert before[other][0].tobytes() == after[other][0].tobytes() and before[other][1] == after[other][1], (name, other)
        ctx.set_profiling(False)
        _call(ctx, pr, "gain_marginal_dense", fam)
        ms, flops = ctx.gain_marginal_profile()
        assert ms.shape == (9,) and (ms == 0).all() and flops > 0, (ms, flops)
