"""The index arithmetic of the fused gather + crop for frame stacks (serl_amd/csrc/stack_index.h: workgroup -> frame, the frame's
source in the packed window or the ring, its crop-table entry and its destination) on the CPU against NumPy.  The header is
compiled, with the host address and undefined-behaviour sanitizers, into the stand-alone program tests/stack_index_main.cpp,
which also touches memory at every index it computes; a sanitizer report ends the child with a non-zero status."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle.replay_oracle import ReplayOracle

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "serl_amd", "csrc")


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ is not on PATH")
    exe = str(tmp_path_factory.mktemp("stack_index") / "stack_index_main")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(HERE, "stack_index_main.cpp"), "-o", exe])

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out = [ln.split() for ln in r.stdout.splitlines()]
        assert len(out) == len(lines), r.stdout
        return out
    return run


GEOMETRIES = [(1, 1, 6, 2), (3, 1, 5, 1), (1, 2, 6, 2), (2, 3, 5, 2), (3, 4, 7, 4), (5, 2, 1, 3)]    # (parts, T, batch, n_cam)


def test_workgroup_decode_matches_numpy(ask):
    outs = ask([f"jobs {p} {T} {B} {nc}" for p, T, B, nc in GEOMETRIES])
    for (parts, T, B, nc), out in zip(GEOMETRIES, outs):
        assert out[0] == "jobs" and out[-1] == "once", out[-1]
        got = np.array([[int(v) for v in tok.split(":")] for tok in out[1:-1]], np.int64)
        n = 2 * nc * B * T * parts
        assert got.shape == (n, 8)
        which, cam, i, t, part = np.unravel_index(np.arange(n), (2, nc, B, T, parts))       # part fastest
        assert np.array_equal(got[:, :5], np.stack([part, t, i, cam, which], 1))
        # out_frames u8[2][n_cam][batch][T][frame]; crop table int32[batch*T][2]: frame (b, t) takes entry b*T + t
        assert np.array_equal(got[:, 5], np.ravel_multi_index((which, cam, i, t), (2, nc, B, T)))
        assert np.array_equal(got[:, 6], i * T + t) and got[:, 6].max() == B * T - 1
        # _unpack: observation frame t = packed frame t, next frame t = packed frame t + 1 of u8[batch][T+1][frame]
        assert np.array_equal(got[:, 7], i * (T + 1) + which + t) and got[:, 7].max() == B * (T + 1) - 1
        if T == 1:      # the single-frame decode it replaces: (part, i, cam, which) and ((which * n_cam + cam) * batch + i)
            w1, c1, i1, p1 = np.unravel_index(np.arange(n), (2, nc, B, parts))
            assert np.array_equal(got[:, [0, 2, 3, 4]], np.stack([p1, i1, c1, w1], 1))
            assert np.array_equal(got[:, 5], (w1 * nc + c1) * B + i1) and np.array_equal(got[:, 6], i1)


@pytest.mark.parametrize("T,cap", [(1, 8), (2, 16), (3, 64), (4, 9)])
def test_window_slots_match_the_replay_oracle(ask, T, cap):
    o = ReplayOracle(("a",), 1, 1, 1, T, 1, 1, cap)
    o.frames["a"][:, 0, 0, 0] = np.arange(cap) % 251          # a slot is recognisable by its frame
    idx = np.arange(cap)
    idx = idx[(idx >= T) | (idx + cap - 2 * T >= 0)]          # every slot whose window numpy can index (negative ones wrap)
    outs = ask([f"window {i} {T} {cap}" for i in idx])
    win = o.gather(idx)["observations"]["a"][:, :, 0, 0, 0]  # (n, T+1): the slots the reference reads
    for row, out in zip(win, outs):
        slots = np.array(out[1:], np.int64)
        assert out[0] == "window" and slots.shape == (T + 1,) and slots.min() >= 0 and slots.max() < cap
        assert np.array_equal(slots % 251, row)
