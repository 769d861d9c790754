"""cafe_gain_leaf_predictive and its debug entry are exported and declared, and the fused kernel of gain_dense.hip uses no scratch
memory and spills no vector register (the compiler's resource remarks of a gfx950 cross-compile; CPU only, skips without hipcc)."""
import os

from helpers import CSRC, kernel_resources


def test_the_entries_are_exported():
    from cafexp_amd import capi
    lib = capi.load()
    header = open(os.path.join(os.path.dirname(CSRC), "..", "include", "cafe_mi355x.h")).read()
    for name in ("cafe_gain_leaf_predictive", "cafe_debug_gain_predictive"):
        assert name in capi.EXPORTS and getattr(lib, name) and "int %s(" % name in header
    assert hasattr(capi.Context, "gain_leaf_predictive") and hasattr(capi.Context, "gain_predictive_profile")


def test_the_fused_kernel_runs_without_scratch():
    kernels = {k: v for k, v in kernel_resources("gain_dense.hip").items() if "gain_predictive_dense_" in k}
    assert len(kernels) == 1 and "gain_predictive_dense_leaf_kernel" in next(iter(kernels)), sorted(kernels)
    for k, res in kernels.items():
        print(k, res.get("VGPRs"), res.get("AGPRs"), res.get("LDS Size"), res.get("Occupancy"))
        assert res["ScratchSize"] == 0 and res["VGPRs Spill"] == 0, (k, res)
