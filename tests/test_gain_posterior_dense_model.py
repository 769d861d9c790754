"""cafe_gain_posterior_dense and its debug entry are exported, and no kernel of the down pass in gain_dense.hip uses scratch
memory or spills a vector register (the compiler's resource remarks of a gfx950 cross-compile; CPU only, skips without hipcc)."""
import os

from helpers import CSRC, kernel_resources

KERNELS = ["gain_posterior_dense_%s_kernel" % k for k in ("weights", "gemm_t", "interior", "leaf")]


def test_the_entries_are_exported():
    from cafexp_amd import capi
    lib = capi.load()
    for name in ("cafe_gain_posterior_dense", "cafe_debug_gain_dense_posterior"):
        assert name in capi.EXPORTS and getattr(lib, name)
    assert "int cafe_gain_posterior_dense(" in open(os.path.join(os.path.dirname(CSRC), "..", "include", "cafe_mi355x.h")).read()
    assert hasattr(capi.Context, "gain_posterior_dense") and hasattr(capi.Context, "gain_dense_posterior_profile")


def test_every_down_kernel_runs_without_scratch():
    kernels = {k: v for k, v in kernel_resources("gain_dense.hip").items() if "gain_posterior_dense_" in k}
    for name in KERNELS:
        assert any(name in k for k in kernels), name
    assert len(kernels) == len(KERNELS), sorted(kernels)
    for k, res in sorted(kernels.items()):
        print(k, res.get("VGPRs"), res.get("AGPRs"), res.get("LDS Size"), res.get("Occupancy"))
        assert res["ScratchSize"] == 0 and res["VGPRs Spill"] == 0, (k, res)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "$(NO_PK32) -c gain_dense.hip,gain_posterior_dense_,0,0)" in mk[mk.index("\ncheck:"):]
