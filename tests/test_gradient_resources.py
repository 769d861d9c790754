"""The kernels of gradient.hip -- the root, scan, weighted-dot, leaf-filter, leaf-sum and finish kernels of
cafe_score_gradient -- keep their recurrences in registers (the leaf filter its three tiles in LDS).  Cross-compile the file
for gfx950 (CPU only) and read the compiler's resource remarks: no kernel may use scratch or spill vector registers (the
rule `make check` applies).  The GEMM is marginal.hip's, pinned by tests/test_marginal_resources.py."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cafexp_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = ["gradient_root_kernel", "gradient_scan_kernel", "gradient_dot_kernel", "gradient_leaf_filter_kernel", "gradient_leaf_kernel",
           "gradient_finish_kernel"]


def _flags():
    with open(os.path.join(CSRC, "Makefile")) as f:
        line = next(ln for ln in f if ln.startswith("FLAGS"))
    return line.split(":=", 1)[1].replace("$(ARCH)", "gfx950").split()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_every_kernel_runs_without_scratch(tmp_path):
    r = subprocess.run([HIPCC] + _flags() + ["-Rpass-analysis=kernel-resource-usage", "-c", "gradient.hip", "-o", str(tmp_path / "g.o")],
                       cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/lane\])?: (\d+)", line)
        if m and name:
            kernels[name][m.group(1).strip()] = int(m.group(2))
    mine = {k: v for k, v in kernels.items() if "gradient_" in k}
    for k in KERNELS:
        assert any(k in n for n in mine), k
    assert len(mine) == len(KERNELS), sorted(mine)
    for k, res in mine.items():
        assert res["ScratchSize"] == 0, (k, res)
        assert res["VGPRs Spill"] == 0, (k, res)
