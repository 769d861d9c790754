"""cafe_score_gain is exported under ABI version 3, and no kernel of gain_dense.hip -- the twelve widths of the matrix build, the
product, the GEMM, the root kernel -- uses scratch memory or spills a vector register: what `make check` holds the file to,
read from the compiler's resource remarks of a gfx950 cross-compile (CPU only; skips without hipcc)."""
import os

from helpers import CSRC, kernel_resources
from test_per_family_shapes import WIDTHS


def test_the_entry_is_exported():
    from cafexp_amd import capi
    lib = capi.load()
    assert lib.cafe_abi_version() == 3
    for name in ("cafe_score_gain", "cafe_debug_gain_dense"):
        assert name in capi.EXPORTS and getattr(lib, name)
    assert "int cafe_score_gain(" in open(os.path.join(os.path.dirname(CSRC), "..", "include", "cafe_mi355x.h")).read()


def test_every_dense_kernel_runs_without_scratch():
    kernels = {k: v for k, v in kernel_resources("gain_dense.hip").items() if "gain_dense_" in k}
    for E in WIDTHS:
        assert any("gain_dense_build_kernelILi%dEEE" % E in k for k in kernels), E
    for name in ("gain_dense_product_kernel", "gain_dense_gemm_kernel", "gain_dense_root_kernel"):
        assert any(name in k for k in kernels), name
    assert len(kernels) == len(WIDTHS) + 3, sorted(kernels)
    for k, res in sorted(kernels.items()):
        print(k, res.get("VGPRs"), res.get("AGPRs"), res.get("LDS Size"), res.get("Occupancy"))
        assert res["ScratchSize"] == 0 and res["VGPRs Spill"] == 0, (k, res)


def test_makefile_builds_and_checks_the_file():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "gain_dense.hip" in next(ln for ln in mk.splitlines() if ln.startswith("SRC")).split()
    check = mk[mk.index("\ncheck:"):]
    assert "gain_dense.hip" in check.splitlines()[1].split()
    assert "-c gain_dense.hip,gain_dense_,0,0)" in check
