"""The kernels of marginal.hip -- the fp64 MFMA GEMM with its 8 accumulator tiles and register prefetch, the product, root,
column-sum, leaf and summary kernels -- keep everything in registers.  Cross-compile the file for gfx950 (CPU only) and read
the compiler's resource remarks: no kernel may use scratch or spill vector registers (the rule `make check` applies)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cafexp_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SMALL = ["marginal_product_kernel", "marginal_root_kernel", "marginal_colsum_kernel", "marginal_leaf_kernel", "marginal_summary_kernel",
         "marginal_leaf_summary_kernel"]


def _flags():
    with open(os.path.join(CSRC, "Makefile")) as f:
        line = next(ln for ln in f if ln.startswith("FLAGS"))
    return line.split(":=", 1)[1].replace("$(ARCH)", "gfx950").split()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_every_kernel_runs_without_scratch(tmp_path):
    r = subprocess.run([HIPCC] + _flags() + ["-Rpass-analysis=kernel-resource-usage", "-c", "marginal.hip", "-o", str(tmp_path / "m.o")],
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
    mine = {k: v for k, v in kernels.items() if "marginal_" in k}
    gemm = [k for k in mine if "marginal_gemm_kernel" in k]
    assert len(gemm) == 4, sorted(gemm)                      # up (store, multiply), down, split
    for k in SMALL:
        assert any(k in n for n in mine), k
    assert len(mine) == len(gemm) + len(SMALL), sorted(mine)
    for k, res in mine.items():
        assert res["ScratchSize"] == 0, (k, res)
        assert res["VGPRs Spill"] == 0, (k, res)
