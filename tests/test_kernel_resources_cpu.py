"""CPU: scripts/kernel_resources.py --check -- the trunk launches of the flagship line stay within their register budget without
scratch, and the update-chain kernels fit into what two resident trunk workgroups leave per SIMD (DESIGN.md sections 4 and 8).
Compiles two files for gfx950 with hipcc's resource remarks; no link, no GPU.

The tightest entries are conv_dma_f16x3_kernel<2, 0, true> (b1_conv0, b2_conv0) and <2, 2, true> (b3_conv0), the 128 x 128 ring
kernel with the fused projection: 215 registers under a cap of 216, and free of scratch only because they are compiled without the
residual epilogues that a conv0 never takes (profiles/ring_proj_isa.txt; profiles/README.md, topmost section)."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="session")
def resource_check():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc is not installed")
    return subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_resources.py"), "--check"], stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True, env={**os.environ, "HIPCC": HIPCC})


def test_flagship_kernels_are_within_their_register_budgets(resource_check):
    print(resource_check.stdout)
    assert resource_check.returncode == 0, resource_check.stdout[-3000:]
    assert "over budget" not in resource_check.stdout
