"""cafe_gain_marginal_dense and its debug entry are exported and declared, its kernels use no scratch memory (the compiler's resource
remarks of a gfx950 cross-compile; skips without hipcc), and -- on the longdouble reference alone -- the inputs of
tests/test_gain_marginal_gpu.py tell the right split at the diagonal from its three nearest mistakes and keep the margins that make
the GPU test's integer comparisons exact.  CPU only."""
import os

import numpy as np
import pytest

import gain_marginal_ref as GM
from helpers import CSRC, kernel_resources


def test_the_entries_are_exported():
    from cafexp_amd import capi
    lib = capi.load()
    header = open(os.path.join(os.path.dirname(CSRC), "..", "include", "cafe_mi355x.h")).read()
    for name in ("cafe_gain_marginal_dense", "cafe_debug_gain_marginal"):
        assert name in capi.EXPORTS and getattr(lib, name) and "int %s(" % name in header
    assert hasattr(capi.Context, "gain_marginal_dense") and lib.cafe_abi_version() == 3 and "#define CAFE_ABI_VERSION 3" in header


def test_the_kernels_run_without_scratch():
    kernels = {k: v for k, v in kernel_resources("gain_dense.hip").items() if "gain_marginal_" in k}
    assert len(kernels) == 5 and any("gain_marginal_dense_split_kernel" in k for k in kernels), sorted(kernels)
    for k, res in kernels.items():
        assert res["ScratchSize"] == 0 and res["VGPRs Spill"] == 0, (k, res)


@pytest.mark.parametrize("case", GM.CASES, ids=str)
def test_the_inputs_tell_the_split_from_its_mistakes_and_keep_their_margins(case):
    pb, pr = GM.problem(*case)
    fam = list(range(pb.n_families)) + [-1]
    right = GM.table(pb, fam, GM.RATES, pr.prior, GM.ABSENT, GM.LEVEL, pr.error_model)
    assert np.isfinite(right["lnl"]).all() and right["lnl"].min() > -600       # inside fp64 with room: the plain mode serves them
    assert right["cdf_gap"].min() > 1e-9 and right["top_gap"].min() > 1e-9
    for key in ("p_increase", "p_decrease", "p_same"):
        assert np.nanmax(right[key]) > 1e-6, key
    assert np.nanmax(right["p_same"]) > 0.3 and GM.RATES[0] != GM.RATES[1]
    assert np.nanmax(np.abs(right["p_increase"] + right["p_decrease"] + right["p_same"] - 1)) < 1e-15      # the three are the whole joint
    for wrong in GM.WRONG:
        other = GM.table(pb, fam, GM.RATES, pr.prior, GM.ABSENT, GM.LEVEL, pr.error_model, wrong)
        assert max(np.nanmax(np.abs(other[key] - right[key])) for key in GM.DOUBLES) > 1e-6, wrong
