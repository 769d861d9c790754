"""cafe_gain_score_gradient and its debug entry are exported, declared and bound, and exactly its six kernels exist in gain_dense.hip
and use no scratch memory and spill no register (the compiler's resource remarks of a gfx950 cross-compile).  CPU only."""
import os

from helpers import CSRC, kernel_resources

KERNELS = ("outside2", "toeplitz", "interior", "filter", "lambda", "leaf")


def test_the_entries_are_exported_and_the_kernels_run_without_scratch():
    from cafexp_amd import capi
    lib = capi.load()
    header = open(os.path.join(os.path.dirname(CSRC), "..", "include", "cafe_mi355x.h")).read()
    for name in ("cafe_gain_score_gradient", "cafe_debug_gain_gradient"):
        assert name in capi.EXPORTS and getattr(lib, name) and "int %s(" % name in header
    assert hasattr(capi.Context, "gain_score_gradient") and hasattr(capi.Context, "gain_gradient_profile") and lib.cafe_abi_version() == 3
    kernels = {k: v for k, v in kernel_resources("gain_dense.hip").items() if "gain_gradient_" in k}
    assert len(kernels) == len(KERNELS) and all(any("gain_gradient_%s_kernel" % n in k for k in kernels) for n in KERNELS), sorted(kernels)
    for k, res in kernels.items():
        assert res["ScratchSize"] == 0 and res["VGPRs Spill"] == 0, (k, res)
