"""The bookkeeping of the fused GroupNorm epilogues' statistics exchange (serl_amd/csrc/gn_exchange.h: granule packing, the pass
epoch, the records a layer needs, a tile's record and its peers') on the CPU against NumPy.  The header is compiled, with the host
address and undefined-behaviour sanitizers, into the stand-alone program tests/gn_exchange_main.cpp, which also writes and reads
every record at the places it computes; a sanitizer report ends the child with a non-zero status."""
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "serl_amd", "csrc")


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ is not on PATH")
    exe = str(tmp_path_factory.mktemp("gn_exchange") / "gn_exchange_main")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(HERE, "gn_exchange_main.cpp"), "-o", exe])

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out = [ln.split() for ln in r.stdout.splitlines()]
        assert len(out) == len(lines), r.stdout
        return out
    return run


def test_epoch_is_never_zero_and_clears_at_the_start_and_at_the_wrap(ask):
    prev = [0, 1, 2, 12345, 2**31 - 1, 2**31, 2**32 - 2, 2**32 - 1]
    outs = ask([f"epoch {p}" for p in prev])
    for p, out in zip(prev, outs):
        nxt, clear = int(out[1]), int(out[2])
        assert out[0] == "epoch" and 1 <= nxt < 2**32
        if p in (0, 2**32 - 1):       # no pass yet (the memory holds anything) / the count wraps: zero the records, start at 1
            assert (nxt, clear) == (1, 1)
        else:
            assert (nxt, clear) == (p + 1, 0)
    # a run of passes: consecutive tags differ, and a tag comes back only behind a clear
    e, seen = 2**32 - 4, []
    for _ in range(8):
        out = ask([f"epoch {e}"])[0]
        e = int(out[1])
        seen.append((e, int(out[2])))
    assert seen == [(2**32 - 3, 0), (2**32 - 2, 0), (2**32 - 1, 0), (1, 1), (2, 0), (3, 0), (4, 0), (5, 0)]


def test_a_granule_keeps_value_and_tag_apart(ask):
    cases = [(0, 1), (0xffffffff, 1), (0x3f800000, 0xffffffff), (0x80000000, 0x80000000), (123, 456)]
    for (v, t), out in zip(cases, ask([f"granule {v} {t}" for v, t in cases])):
        assert out == ["granule", str(v), str(t)]


# (images, P, Cout, tile rows, tile columns): the row-slab kernels' 256 x 64 tiles at 128 x 128 / 128 x 64 / 256 x 128 frames, the
# LDS-DMA kernel's 128 x 128 and 128 x 64 tiles on b1_conv0 and on a stage-2 map of 256 pixels, one row tile per image
LAUNCHES = [(3, 1024, 64, 256, 64), (5, 512, 64, 256, 64), (2, 2048, 64, 256, 64), (3, 512, 128, 256, 64), (4, 256, 128, 128, 128),
            (4, 256, 128, 128, 64), (2, 256, 256, 128, 128), (2, 256, 256, 128, 64), (3, 128, 128, 128, 64)]


def test_every_tile_finds_the_records_of_its_image_and_column(ask):
    outs = ask([f"launch {n} {P} {C} {tr} {tc} {7 + i}" for i, (n, P, C, tr, tc) in enumerate(LAUNCHES)])
    for (n, P, C, tr, tc), out in zip(LAUNCHES, outs):
        rows, tiles_n = P // tr, C // tc
        assert out[0] == "launch" and out[-1] == "complete", out[-1]
        got = np.array([[int(v) for v in tok.split(":")] for tok in out[1:-1]], np.int64)
        assert got.shape == (n * rows * tiles_n, 4)
        image, r, bn = np.unravel_index(np.arange(len(got)), (n, rows, tiles_n))      # tile = (image * rows + r) * tiles_n + bn
        assert np.array_equal(got[:, 0], np.ravel_multi_index((image, 0 * r, bn), (n, rows, tiles_n)))
        assert np.array_equal(got[:, 1], np.full(len(got), tiles_n)) and np.array_equal(got[:, 2], np.full(len(got), rows))
        assert np.array_equal(got[:, 3], r)
        assert np.array_equal(got[:, 0] + got[:, 3] * got[:, 1], np.arange(len(got)))   # its own record is one of them


def test_a_layer_has_a_record_for_every_tile_that_can_exchange(ask):
    shapes = [(P, C) for P in (16, 64, 100, 128, 256, 441, 512, 1024, 2048, 4096) for C in (64, 128, 256, 512)]
    for (P, C), out in zip(shapes, ask([f"capacity {P} {C}" for P, C in shapes])):
        cap = int(out[1])
        assert out[0] == "capacity" and cap >= 0
        for tr, tc in ((256, 64), (128, 128), (128, 64)):      # tiles that lie in one image
            if P % tr == 0 and C % tc == 0:
                assert cap >= (P // tr) * (C // tc), (P, C, tr, tc, cap)
