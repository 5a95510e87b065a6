"""The launch planner of the batched replay insert (serl_amd/csrc/replay_batch.h) on the CPU.  tests/replay_batch_main.cpp holds
the proof: a host model of the slots fed sequentially (ReplayIndex::plan_insert per transition) and through the planner's
launches, each launch executed in reverse and in shuffled op order against a snapshot taken before it; slots and bookkeeping
must agree after every payload and every launch must satisfy the cut conditions.  The program is compiled with the host address
and undefined-behaviour sanitizers and run as a child process; a sanitizer report ends it with a non-zero status, which fails
the test."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "serl_amd", "csrc")


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ is not on PATH")
    exe = str(tmp_path_factory.mktemp("replay_batch") / "replay_batch_main")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(HERE, "replay_batch_main.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("T", [1, 2, 3, 4, 0], ids=["T1", "T2", "T3", "T4", "frameless"])
def test_launches_equal_sequential_inserts(binary, T):
    """T 1-4 at capacities 3T+2, 11+T and 37, the frameless store at 2, 5 and 16; staging budgets of 1, 3 and 64 entries; payloads
    cycling 1, 2, 7, cap-1, cap and 2*cap+3 transitions; done probability 0.2; at least 2000 transitions per case."""
    out = subprocess.run([binary, str(T)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("ok"), (out.stdout[-2000:], out.stderr[-4000:])
    cases = re.findall(r"^case cap=(\d+) frames=(\d) T=(\d) budget=(\d+) release=(\d) transitions=(\d+) launches=(\d+)$", out.stdout, re.M)
    caps = [3 * T + 2, 11 + T, 37] if T else [2, 5, 16]
    want = {(cap, int(T != 0), T or 1, budget, release) for cap in caps for budget in (1, 3, 64) for release in (0, 1)}
    assert {tuple(int(x) for x in c[:5]) for c in cases} == want
    assert all(int(c[5]) >= 2000 and int(c[6]) > 0 for c in cases)
    # a budget of one entry puts every slot write into a launch of its own; a larger one must actually batch
    by = {tuple(int(x) for x in c[:5]): int(c[6]) for c in cases}
    for cap in caps:
        assert by[(cap, int(T != 0), T or 1, 64, 0)] < by[(cap, int(T != 0), T or 1, 1, 0)]


def test_the_planner_header_has_no_hip_in_it():
    txt = open(os.path.join(CSRC, "replay_batch.h")).read()
    assert "hip" not in re.sub(r"//.*", "", txt).lower()
