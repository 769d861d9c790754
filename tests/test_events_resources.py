"""The kernels of events.hip -- the scan that writes both scanned panels and the leaf filter of cafe_expected_events -- keep
their recurrences in registers (the leaf filter its three tiles in LDS).  Cross-compile the file for gfx950 (CPU only) and read
the compiler's resource remarks: no kernel may use scratch or spill vector registers (the rule `make check` applies).  The
root, weighted-dot, leaf-sum and finish kernels are gradient.hip's, pinned by tests/test_gradient_resources.py; the GEMM is
sum_product.hip's, pinned by tests/test_sum_product_resources.py."""
from helpers import kernel_resources

KERNELS = ["events_scan_kernel", "events_leaf_filter_kernel"]


def test_every_kernel_runs_without_scratch():
    kernels = kernel_resources("events.hip")
    mine = {k: v for k, v in kernels.items() if "events_" in k}
    for k in KERNELS:
        assert any(k in n for n in mine), k
    assert len(mine) == len(KERNELS), sorted(mine)
    for k, res in mine.items():
        assert res["ScratchSize"] == 0, (k, res)
        assert res["VGPRs Spill"] == 0, (k, res)
