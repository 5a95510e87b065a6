"""The update chain's Dense -> LayerNorm -> activation layer description (serl_amd/csrc/dense_layer.h) on the CPU.
tests/dense_layer_main.cpp holds the proof: for the camera bottleneck (4096 -> 256, 1 and 3 cameras, output a column slice of a
wider row), the proprio branch (19 -> 64), critic layers 1 and 2 (70.. -> 128 -> 128, 2 and 3 members, a shared input against a
per-member one, one output block per member) and policy layers 1 and 2, on 1, 5 and 65 rows, the forward GEMM, LayerNorm forward,
LayerNorm backward, column-sum, kernel-gradient and input-gradient arguments derived from the description equal, field by field,
the explicit positional form of every former call site.  The program is compiled with the host address and undefined-behaviour
sanitizers and run as a child process; a sanitizer report ends it with a non-zero status, which fails the test."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "serl_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH") or "/opt/rocm"


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ is not on PATH")
    if not os.path.exists(os.path.join(ROCM, "include", "hip", "hip_runtime.h")):
        pytest.skip("the HIP headers are not installed")
    exe = str(tmp_path_factory.mktemp("dense_layer") / "dense_layer_main")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"), "-I", CSRC,
                           os.path.join(HERE, "dense_layer_main.cpp"), "-o", exe])
    return exe


def test_derived_arguments_equal_the_explicit_call_sites(binary):
    out = subprocess.run([binary], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("ok"), (out.stdout[-2000:], out.stderr[-4000:])
    cases = set(re.findall(r"^case (cams=\d+ ens=\d+ rows=\d+) batch=\d+ ok$", out.stdout, re.M))
    assert cases == {f"cams={c} ens={e} rows={r}" for c in (1, 3) for e in (2, 3) for r in (1, 5, 65)}


def test_the_header_has_no_device_code_in_it():
    txt = re.sub(r"//.*", "", open(os.path.join(CSRC, "dense_layer.h")).read())
    assert "__global__" not in txt and "__device__" not in txt and "hipLaunch" not in txt
