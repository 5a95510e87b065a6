"""The replay store's host bookkeeping (serl_amd/csrc/replay_index.h: slot bookkeeping, insert plans, PCG64 index sampler) on the
CPU, bit-exact against the reference-generated golden fixtures and the live NumPy oracle.  The header is compiled once, with the
host address and undefined-behaviour sanitizers, into the stand-alone program tests/replay_index_main.cpp and driven through its
line protocol as a child process; any sanitizer report ends the child with a non-zero status, which fails the test."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import load_case, stream_for
from oracle.replay_oracle import PlainReplayOracle, ReplayOracle

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "serl_amd", "csrc")
CASES = ["small_wrap", "small_nowrap", "one_cam", "wrap_quirk"]
M64 = (1 << 64) - 1


@pytest.fixture(scope="session")
def binary(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ is not on PATH")
    exe = str(tmp_path_factory.mktemp("replay_index") / "replay_index_main")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(HERE, "replay_index_main.cpp"), "-o", exe])
    return exe


class Index:
    """One child process = one ReplayIndex."""

    def __init__(self, exe, cap, has_frames, T):
        self.p = subprocess.Popen([exe], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert self.ask(f"create {cap} {int(has_frames)} {T}") == ["ok"]

    def ask(self, line):
        self.p.stdin.write(line + "\n")
        self.p.stdin.flush()
        out = self.p.stdout.readline()
        assert out, f"the program ended at {line!r}:\n{self.p.stderr.read()}"
        return out.split()

    def seed(self, gen):
        st = gen.bit_generator.state
        s, inc = st["state"]["state"], st["state"]["inc"]
        assert self.ask(f"seed {s >> 64} {s & M64} {inc >> 64} {inc & M64} {st['has_uint32']} {st['uinteger']}") == ["ok"]

    def insert(self, done):
        """-> the plan as [(kind, dst, arg)]"""
        out = self.ask(f"insert {int(bool(done))}")
        assert out[0] == "plan"
        return [(k, int(d), int(a)) for k, d, a in (op.split(":") for op in out[1:])]

    def indices(self, line):
        """-> the index vector, or the status name"""
        out = self.ask(line)
        return np.array(out[1:], np.int64) if out[0] == "idx" else out[1]

    def sample(self, B):
        return self.indices(f"sample {B}")

    def revalidate(self, idx):
        return self.indices("revalidate " + " ".join(str(int(i)) for i in idx))

    def dump(self):
        out = self.ask("dump")
        assert out[0] == "dump" and len(out) == 12
        return dict(size=int(out[1]), insert_index=int(out[2]), insert_count=int(out[3]), first=bool(int(out[4])),
                    valid=np.array([c == "1" for c in out[5]]), rng=[int(w) for w in out[6:10]], has_uint32=int(out[10]),
                    uinteger=int(out[11]))

    def close(self):
        _, err = self.p.communicate()
        assert self.p.returncode == 0, f"exit status {self.p.returncode}:\n{err}"


@pytest.fixture
def make(binary):
    made = []

    def _make(cap, has_frames=True, T=1):
        made.append(Index(binary, cap, has_frames, T))
        return made[-1]
    yield _make
    for ix in made:
        ix.close()


def assert_rng_equals(d, gen):
    st = gen.bit_generator.state
    s, inc = st["state"]["state"], st["state"]["inc"]
    assert d["rng"] == [s >> 64, s & M64, inc >> 64, inc & M64]
    assert d["has_uint32"] == st["has_uint32"] and d["uinteger"] == st["uinteger"]


@pytest.mark.parametrize("name", CASES)
def test_golden_cases(make, name):
    z, m = load_case(name)
    ix = make(m["cap"], len(m["keys"]) > 0, m["T"])
    for tr in stream_for(m):
        ix.insert(tr["dones"])
    d = ix.dump()
    assert d["size"] == int(z["size"]) and d["insert_index"] == int(z["insert_index"])
    assert (d["valid"] == z["valid"]).all()
    ix.seed(np.random.default_rng(m["rseed"]))
    for s in range(m["ns"]):
        assert (ix.sample(m["B"]) == z[f"idx_{s}"]).all(), "index stream must be bit-exact"


def done_flags(seed, n):
    """Episode lengths drawn from 1..7; two episodes of one step follow each other, so two transitions in a row are `done`."""
    lens = [int(x) for x in np.random.default_rng(seed).integers(1, 8, size=n)]
    lens[2] = lens[3] = 1
    flags = [t == ln - 1 for ln in lens for t in range(ln)]
    assert any(a and b for a, b in zip(flags, flags[1:]))
    return flags


def frame_transition(T, done):
    """Frames of 1x16x1 whose first byte says which frame it is: observation frame t holds t + 1, the last next frame 100."""
    obs = np.zeros((T, 1, 16, 1), np.uint8)
    obs[:, 0, 0, 0] = np.arange(1, T + 1)
    nobs = np.full((T, 1, 16, 1), 100, np.uint8)
    st = np.zeros((T, 1), np.float32)
    return {"observations": {"state": st, "img": obs}, "next_observations": {"state": st, "img": nobs},
            "actions": np.zeros(1, np.float32), "rewards": np.float32(0), "masks": np.float32(1 - done), "dones": bool(done)}


def instrument(o):
    """-> (writes, copies): the slots `o` writes, in order, and the (dst, src) of its wrap re-inserts"""
    writes, copies = [], []
    raw, copy = o._raw_insert, o._copy_slot_to_head

    def raw_insert(*a):
        writes.append(o.insert_index)
        return raw(*a)

    def copy_slot_to_head(src):
        copies.append((o.insert_index, src))
        return copy(src)
    o._raw_insert, o._copy_slot_to_head = raw_insert, copy_slot_to_head
    return writes, copies


@pytest.mark.parametrize("cap", [17, 24])
@pytest.mark.parametrize("T", [1, 2, 3])
def test_generated_streams_match_oracle(make, T, cap):
    o = ReplayOracle(("img",), 1, 16, 1, T, 1, 1, cap)
    o.seed(11)
    ix = make(cap, True, T)
    ix.seed(o.rng)
    writes, copies = instrument(o)
    total = 0
    for n, done in enumerate(done_flags(5, 24)):
        del writes[:], copies[:]
        o.insert(frame_transition(T, done))
        plan = ix.insert(done)
        assert len(plan) <= 2 * T + 1
        assert [dst for _, dst, _ in plan] == writes
        assert [(dst, src) for kind, dst, src in plan if kind == "c"] == copies
        for kind, dst, t in plan:   # the frame the plan names is the frame the oracle stored
            if kind != "c":
                assert o.frames["img"][dst][0, 0, 0] == (t + 1 if kind == "o" else 100) and (kind == "o" or t == T - 1)
        total += len(writes)
        d = ix.dump()
        assert d["size"] == o.size and d["insert_index"] == o.insert_index and d["first"] == o.first and d["insert_count"] == total
        assert (d["valid"] == o.valid).all()
        if n % 5 == 4:
            assert (ix.sample(33) == o.sample_indices(33)).all()
    assert total >= 3 * cap, "the stream must wrap the ring at least three times"
    assert_rng_equals(ix.dump(), o.rng)


def test_plain_store_matches_oracle(make):
    cap = 17
    o = PlainReplayOracle(1, 1, cap)
    o.seed(3)
    ix = make(cap, False, 1)
    ix.seed(o.rng)
    z = np.zeros(1, np.float32)
    for n, done in enumerate(done_flags(9, 20)):
        head = o.insert_index
        o.insert({"observations": z, "next_observations": z, "actions": z, "rewards": 0.0, "masks": 1.0, "dones": done})
        assert ix.insert(done) == [("n", head, 0)]
        d = ix.dump()
        assert d["size"] == o.size and d["insert_index"] == o.insert_index and d["insert_count"] == n + 1
        assert d["valid"][:o.size].all() and not d["valid"][o.size:].any()
        if n % 5 == 4:
            assert (ix.sample(33) == o.sample_indices(33)).all()
    assert n + 1 >= 3 * cap
    assert_rng_equals(ix.dump(), o.rng)


def test_revalidate_redraws_stale_indices_in_place(make):
    T, cap = 2, 24
    o = ReplayOracle(("img",), 1, 16, 1, T, 1, 1, cap)
    o.seed(21)
    ix = make(cap, True, T)
    ix.seed(o.rng)
    flags = done_flags(7, 20)
    for done in flags[:30]:
        o.insert(frame_transition(T, done))
        ix.insert(done)
    idx = ix.sample(64)
    assert (idx == o.sample_indices(64)).all()
    for done in flags[30:40]:
        o.insert(frame_transition(T, done))
        ix.insert(done)
    assert not o.valid[idx].all(), "the inserts must have invalidated a drawn slot"
    want = idx.copy()
    for i in range(len(want)):   # what the rejection loop would have drawn, from the oracle's generator
        while not o.valid[want[i]]:
            want[i] = o.rng.integers(len(o))
    got = ix.revalidate(idx)
    assert (got == want).all() and (got != idx).any()
    assert_rng_equals(ix.dump(), o.rng)
    assert (ix.revalidate(got) == got).all()   # nothing stale: no draw
    assert_rng_equals(ix.dump(), o.rng)


def test_error_statuses(make):
    gen = np.random.default_rng(0)
    ix = make(8, True, 1)
    ix.insert(False)
    assert ix.sample(4) == "not_seeded"
    ix = make(8, True, 1)
    ix.seed(gen)
    assert ix.sample(4) == "empty"
    assert isinstance(ix.sample(0), np.ndarray)
    # slots but no valid one: bookkeeping restored over a mask that marks nothing valid (a store of first-frame slots only)
    assert ix.ask("restore 3 3 3 1") == ["status", "ok"]
    assert ix.sample(4) == "none_valid"
    assert ix.ask("restore 3 4 3 1") == ["status", "inconsistent"] and ix.ask("restore 8 3 3 1") == ["status", "inconsistent"]
    assert ix.dump()["size"] == 3
    ix = make(8, True, 1)
    ix.seed(gen)
    for _ in range(3):
        ix.insert(False)
    size = ix.dump()["size"]
    assert ix.revalidate([1, size]) == "out_of_range" and ix.revalidate([-1]) == "out_of_range"
    assert isinstance(ix.revalidate([size - 1]), np.ndarray)
    assert ix.ask("runs 6 5") == ["runs", "6:2:0", "0:3:2"] and ix.ask("runs 2 3") == ["runs", "2:3:0"]
