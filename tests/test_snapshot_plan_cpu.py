"""The staging layout and the workgroup parts of a parameter snapshot (serl_amd/csrc/snapshot_plan.h) on the CPU.
tests/snapshot_plan_main.cpp holds the proof: for run lengths of 1, 3, 4, 5, 4095, 4096, 4097 and 3*4096+2 floats, several runs per
section and empty sections, the parts tile every run exactly once, vector bodies are 16-byte aligned on both sides, tails are shorter
than four floats, section tags are right and the staging size is the header plus the rounded runs; a host model of the pack kernel then
moves real floats part by part and counts the non-finite ones.  The program is compiled with the host address and
undefined-behaviour sanitizers and run as a child process; a sanitizer report ends it with a non-zero status, which fails the test.

The pack kernel itself is compiled for gfx950 with the compiler's resource remarks (no link, no GPU): it must use no LDS and no
scratch and fit the register budget of the kernels that run beside two resident trunk workgroups (scripts/kernel_resources.py:
80 registers)."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "serl_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ is not on PATH")
    exe = str(tmp_path_factory.mktemp("snapshot_plan") / "snapshot_plan_main")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(HERE, "snapshot_plan_main.cpp"), "-o", exe])
    return exe


def test_parts_tile_every_run_and_the_host_model_copies_them(binary):
    out = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("ok"), (out.stdout[-2000:], out.stderr[-4000:])
    cases = dict(re.findall(r"^case (\S+) runs=\d+ parts=(\d+) ", out.stdout, re.M))
    for n in (1, 3, 4, 5, 4095, 4096, 4097, 3 * 4096 + 2):
        assert int(cases[f"single_{n}"]) == -(-n // 4096)
    assert {"empty", "all_lengths_one_section", "several_runs_per_section", "empty_middle_section", "only_last_section"} <= set(cases)
    assert int(cases["empty"]) == 0


def test_the_plan_header_has_no_device_api_in_it():
    txt = re.sub(r"//.*", "", open(os.path.join(CSRC, "snapshot_plan.h")).read()).lower()
    assert "hip" not in txt and "__global__" not in txt and "__device__" not in txt


def test_the_pack_kernel_needs_no_lds_no_scratch_and_few_registers():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc is not installed")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-c",
                        os.path.join(CSRC, "snapshot.hip"), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    block = p.stderr[p.stderr.index("snapshot_pack_kernel"):]
    val = {k.strip(): int(v) for k, v in re.findall(r"remark:\s+([A-Za-z /\[\]]+?):\s+(\d+)\s+\[-Rpass-analysis", block)}
    assert val["LDS Size [bytes/block]"] == 0 and val["ScratchSize [bytes/lane]"] == 0
    assert val["VGPRs"] + val["AGPRs"] <= 80, val
