"""GPU: save_snapshot / restore_snapshot of the HBM replay stores.  In every case the second store is a FRESH store restored
from the snapshot; it must be the first one -- bookkeeping, valid mask, sampler state, every live slot's bytes -- and stay it
while both go on inserting and sampling.  Integer / byte work: every comparison is exact."""
import itertools
import os
import threading

import numpy as np
import pytest
import torch

from helpers import load_case, make_spaces, stream_for
from oracle.replay_oracle import PlainReplayOracle, ReplayOracle

pytestmark = pytest.mark.gpu
KEYS2 = ("front", "wrist")
GEOMS = {     # capacity 48; W * C = 96 and 144 bytes per row (multiples of 16)
    "two_cam": dict(keys=KEYS2, H=32, W=32, C=3, T=1, S=5, A=3, cap=48),
    "one_cam": dict(keys=("image",), H=32, W=48, C=3, T=1, S=5, A=3, cap=48),
}
B = 16


def _mk(g, **over):
    from serl_amd.data.data_store import MemoryEfficientReplayBufferDataStore
    g = dict(g, **over)
    osp, asp = make_spaces(g["keys"], g["H"], g["W"], g["C"], g["T"], g["S"], g["A"])
    return MemoryEfficientReplayBufferDataStore(osp, asp, g["cap"], image_keys=g["keys"])


def _oracle(g):
    return ReplayOracle(g["keys"], g["H"], g["W"], g["C"], g["T"], g["S"], g["A"], g["cap"])


def _stream(g, ep, seed=11):
    from serl_amd.utils.synthetic import transition_stream
    return transition_stream(g["keys"], g["H"], g["W"], g["C"], g["T"], g["S"], g["A"], ep, seed)


def _restored(g, path, mk=_mk):
    b = mk(g)
    b.restore_snapshot(path)
    return b


def _np(t):
    return t.cpu().numpy()


def _compare(a, b, g, oracle=None):
    """Bookkeeping, mask and generator equal; the next 5 index draws equal; gathers byte-equal (frames) / bit-equal (records);
    one fused gather + crop at fixed offsets byte-equal.  `oracle` (ReplayOracle in the same state, same seed) is drawn from
    and compared in lockstep."""
    from serl_amd.agents.batch import DeviceBatch
    from serl_amd.data.data_store import gather_crop
    assert len(a) == len(b) and a.latest_data_id() == b.latest_data_id() and a.insert_count() == b.insert_count()
    assert (a.valid_mask() == b.valid_mask()).all()
    assert a.rng_state() == b.rng_state()
    if oracle is not None:
        assert len(a) == len(oracle) and a.latest_data_id() == oracle.insert_index and (a.valid_mask() == oracle.valid).all()
    for _ in range(5):
        ia, ib = a.sample_indices(B), b.sample_indices(B)
        assert (ia == ib).all()
        ga, gb = a.gather(ia), b.gather(ib)
        torch.cuda.synchronize()
        for k in g["keys"]:
            assert torch.equal(ga["observations"][k], gb["observations"][k])
        for x, y in ((ga["observations"]["state"], gb["observations"]["state"]),
                     (ga["next_observations"]["state"], gb["next_observations"]["state"])) + tuple(
                         (ga[f], gb[f]) for f in ("actions", "rewards", "masks", "dones")):
            assert _np(x).tobytes() == _np(y).tobytes()
        if oracle is not None:
            assert (ia == oracle.sample_indices(B)).all()
            go = oracle.gather(ia)
            for k in g["keys"]:
                assert (_np(gb["observations"][k]) == go["observations"][k]).all()
            assert (_np(gb["observations"]["state"]) == go["observations"]["state"]).all()
            assert (_np(gb["rewards"]) == go["rewards"]).all() and (_np(gb["dones"]) == go["dones"]).all()
    assert a.rng_state() == b.rng_state()
    rng = np.random.default_rng(3)
    co, cn = (rng.integers(0, 9, size=(B, 2)).astype(np.int32) for _ in range(2))
    outs = []
    for s in (a, b):
        out = DeviceBatch(B, len(g["keys"]), g["H"], g["W"], g["C"], g["S"], g["A"], 0)
        gather_crop([(s, ia.copy())], co, cn, out)
        outs.append(out)
    torch.cuda.synchronize()
    assert torch.equal(outs[0].frames, outs[1].frames)
    for f in ("state", "action", "reward", "mask", "done"):
        assert _np(getattr(outs[0], f)).tobytes() == _np(getattr(outs[1], f)).tobytes()


def _roundtrip(g, transitions, n, tmp_path, more=30, seed=5):
    """insert n -> snapshot -> fresh store restored -> compare; then `more` further inserts into both (and the oracle, which
    so sees the whole uninterrupted sequence) -> compare again."""
    a, o = _mk(g), _oracle(g)
    a.seed(seed)
    o.seed(seed)
    for tr in transitions[:n]:
        a.insert(tr)
        o.insert(tr)
    m = a.save_snapshot(str(tmp_path / "snap"))
    assert m["count"] == a.insert_count() and m["first"] == o.first and m["size"] == len(o)
    assert sum(s["n_slots"] for s in m["segments"]) == min(m["count"], g["cap"])
    b = _restored(g, str(tmp_path / "snap"))
    _compare(a, b, g, o)
    for tr in transitions[n:n + more]:        # a missing `first` flag, a stale host mirror of the records (wrap re-insert) or a
        a.insert(tr)                          # wrong count shows here
        b.insert(tr)
        o.insert(tr)
    _compare(a, b, g, o)


# (episode length, inserts before the snapshot).  Capacity 48, T = 1: an episode of L transitions writes L + 1 slots (its
# first-frame slot first), a wrap inside an episode re-inserts the last slot at the head.
FILLS = {
    "before_first_wrap": (1000, 30),          # 31 slot writes
    "exactly_full": (1000, 47),               # 48 slot writes: size == capacity, head back at 0, wrap not yet taken
    "one_and_a_half_wraps": (1000, 71),
    # episode ends around the wrap point: L = 22 -> episodes fill slots 0-22, 23-45, the third one's first-frame slot is 46
    "done_then_head_at_46": (22, 44),         # 46 slot writes, `first` pending: the next insert writes first-frame 46 + slot 47
    "first_frame_46_full": (22, 45),          # first-frame slot 46 and slot 47 written: full, look-ahead invalidates slot 0
    "first_frame_46_wrapped": (22, 46),       # the wrap re-insert (slot 47 -> 0) taken, slot 1 written, look-ahead at slot 2
    # L = 23 -> episodes fill 0-23, 24-47: the ring is full exactly at a done (the wrap-quirk: no re-insert, first-frame at 0)
    "done_at_ring_end": (23, 46),             # 48 slot writes, `first` pending at the wrap
    "first_frame_at_0": (23, 47),             # first-frame slot 0 after the wrap, slot 1, look-ahead at slot 2
    "done_after_wrap": (24, 70),              # L = 24: the wrap falls inside the second episode, the third one's first-frame slot is 3
}


@pytest.mark.parametrize("fill", sorted(FILLS))
@pytest.mark.parametrize("geom", ["two_cam"])
def test_restored_store_is_the_store(gpu, tmp_path, geom, fill):
    g = GEOMS[geom]
    ep, n = FILLS[fill]
    _roundtrip(g, list(itertools.islice(_stream(g, ep), n + 30)), n, tmp_path)


def test_restored_single_camera_store(gpu, tmp_path):
    g = GEOMS["one_cam"]
    _roundtrip(g, list(itertools.islice(_stream(g, 19), 100)), 70, tmp_path)


def test_restored_wrap_quirk_case(gpu, tmp_path):
    """the insert sequence of tests/golden/replay_wrap_quirk.npz (a valid slot 0 whose window index is negative)"""
    z, m = load_case("wrap_quirk")
    g = dict(m)
    trs = list(stream_for(m))
    a = _mk(g)
    a.seed(m["rseed"])
    for tr in trs:
        a.insert(tr)
    assert (a.valid_mask() == z["valid"]).all() and len(a) == int(z["size"])
    a.save_snapshot(str(tmp_path / "snap"))
    b = _restored(g, str(tmp_path / "snap"))
    for s in range(m["ns"]):                 # the restored store reproduces the reference's own draws and bytes
        idx = b.sample_indices(m["B"])
        assert (idx == z[f"idx_{s}"]).all()
        got = b.gather(idx)
        torch.cuda.synchronize()
        for k in m["keys"]:
            assert (_np(got["observations"][k]) == z[f"frames_{k}_{s}"]).all()
        assert (_np(got["rewards"]) == z[f"rewards_{s}"]).all()
    _roundtrip(g, trs + list(itertools.islice(_stream(g, m["ep"], seed=77), 30)), len(trs), tmp_path / "again")


# ---- the plain store of flat observations, at the geometry of the plain_* cases of tests/test_sac_state_gpu.py
class _Box:
    def __init__(self, shape):
        self.shape = shape


def test_plain_store(gpu, tmp_path):
    from serl_amd.data.data_store import ReplayBufferDataStore
    from serl_amd.utils.synthetic import flat_stream
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "replay_plain_wrap.npz"))
    S, A, cap = [int(x) for x in z["meta"][:3]]
    mk = lambda: ReplayBufferDataStore(_Box((S,)), _Box((A,)), capacity=cap)   # noqa: E731
    trs = list(itertools.islice(flat_stream(S, A, 20, 3), 2 * cap + 40))
    for n in (cap // 2, cap, cap + cap // 2):
        a, o = mk(), PlainReplayOracle(S, A, cap)
        a.seed(9)
        o.seed(9)
        for tr in trs[:n]:
            a.insert(tr)
            o.insert(tr)
        p = str(tmp_path / f"snap{n}")
        a.save_snapshot(p)
        b = mk()
        b.restore_snapshot(p)
        for phase in range(2):
            assert len(a) == len(b) == len(o) and a.latest_data_id() == b.latest_data_id() == o.insert_index
            assert a.insert_count() == b.insert_count() and a.rng_state() == b.rng_state()
            for _ in range(5):
                ia, ib = a.sample_indices(B), b.sample_indices(B)
                assert (ia == ib).all() and (ia == o.sample_indices(B)).all()
                ga, gb, go = a.gather(ia), b.gather(ib), o.gather(ia)
                torch.cuda.synchronize()
                for f in ("observations", "next_observations", "actions", "rewards", "masks", "dones"):
                    assert _np(ga[f]).tobytes() == _np(gb[f]).tobytes() and (_np(gb[f]) == go[f]).all()
            for tr in trs[n:n + 30] if phase == 0 else ():
                a.insert(tr)
                b.insert(tr)
                o.insert(tr)


# ---- incremental saves
def _ring(store, path):
    """every live slot of `store` as host arrays, through a full snapshot of it"""
    from serl_amd.data import snapshot as snap
    store.save_snapshot(str(path))
    m, valid, segs = snap.read_snapshot(str(path))
    r = snap.assemble(m, valid, segs)
    r["state"] = (m["size"], m["insert_index"], m["count"], m["first"], m["rng"])
    return r


def _same_ring(x, y):
    assert x["state"] == y["state"] and (x["valid"] == y["valid"]).all() and (x["written"] == y["written"]).all()
    w = x["written"]
    assert all((p[w] == q[w]).all() for p, q in zip(x["frames"], y["frames"]))
    assert x["records"][w].tobytes() == y["records"][w].tobytes()


def test_incremental_saves(gpu, tmp_path):
    g = GEOMS["two_cam"]
    trs = iter(list(itertools.islice(_stream(g, 1000), 400)))
    a = _mk(g)
    a.seed(2)
    inc = str(tmp_path / "inc")

    def insert(n):
        for tr in itertools.islice(trs, n):
            a.insert(tr)

    insert(30)                                   # 31 slot writes
    m0 = a.save_snapshot(inc)
    insert(20)                                   # 17 slots to the end of the ring, the wrap re-insert, 3 more: 21 slot writes
    m1 = a.save_snapshot(inc, incremental=True)
    assert [s["n_slots"] for s in m1["segments"]] == [31, 21] and m1["segments"][0] == m0["segments"][0]
    _same_ring(_ring(_restored(g, inc), tmp_path / "r1"), _ring(a, tmp_path / "f1"))
    insert(40)                                   # slots 4..43: past the first segment's slots, no wrap inside
    m2 = a.save_snapshot(inc, incremental=True)
    assert m2["segments"][-1]["n_slots"] <= 40 and m2["segments"][-1]["first_count"] == m1["count"]
    assert m2["segments"][:-1] == m1["segments"][-1:]      # the first segment is overwritten whole by the later two: dropped
    b = _restored(g, inc)
    full = str(tmp_path / "full")
    a.save_snapshot(full)                        # one full save taken at the end
    c = _restored(g, full)
    _same_ring(_ring(b, tmp_path / "rb"), _ring(c, tmp_path / "rc"))
    _compare(b, c, g)
    _compare(a, _restored(g, inc), g)
    # an incremental save with nothing new keeps the segments and still rewrites the small metadata
    a.sample_indices(3)
    m3 = a.save_snapshot(inc, incremental=True)
    assert m3["segments"] == m2["segments"] and m3["rng"] != m2["rng"]
    # more than `capacity` slot writes between two saves: the whole ring
    insert(60)
    m4 = a.save_snapshot(inc, incremental=True)
    assert [s["n_slots"] for s in m4["segments"]] == [g["cap"]]
    b = _restored(g, inc)
    _same_ring(_ring(b, tmp_path / "rb2"), _ring(a, tmp_path / "ra2"))
    _compare(a, b, g)
    # incremental into an empty directory is a full save
    m5 = a.save_snapshot(str(tmp_path / "new"), incremental=True)
    assert [s["n_slots"] for s in m5["segments"]] == [g["cap"]]


# ---- refusals
@pytest.mark.parametrize("change", [{"H": 48}, {"W": 48}, {"cap": 64}])
def test_wrong_geometry_is_refused_and_the_store_untouched(gpu, tmp_path, change):
    import ctypes as C
    from serl_amd import _lib
    g = GEOMS["two_cam"]
    a = _mk(g)
    a.seed(1)
    for tr in itertools.islice(_stream(g, 15), 60):
        a.insert(tr)
    a.save_snapshot(str(tmp_path / "snap"))
    g2 = dict(g, **change)
    other = _mk(g2)
    other.seed(4)
    for tr in itertools.islice(_stream(g2, 9, seed=5), 40):
        other.insert(tr)
    idx = other.sample_indices(B)
    before, state = other.gather(idx), (len(other), other.latest_data_id(), other.insert_count(), other.rng_state())
    mask = other.valid_mask()
    with pytest.raises(ValueError, match="manifest.json"):
        other.restore_snapshot(str(tmp_path / "snap"))
    # the C entry point refuses the same on its own
    meta = _lib.SerlRbMeta()
    _lib.check(_lib.lib().serl_rb_export_meta(a.handle, C.byref(meta)))
    assert _lib.lib().serl_rb_import_meta(other.handle, C.byref(meta)) == -1        # SERL_ERR_INVALID
    assert b"geometry" in _lib.lib().serl_last_error()
    _lib.check(_lib.lib().serl_rb_export_meta(other.handle, C.byref(meta)))
    meta.insert_count += 1                                                          # inconsistent bookkeeping
    assert _lib.lib().serl_rb_import_meta(other.handle, C.byref(meta)) == -1
    for bad in ((-1, 1), (g2["cap"], 1), (0, g2["cap"] + 1), (0, -1)):               # slot ranges outside the ring
        assert _lib.lib().serl_rb_export_slots(other.handle, bad[0], bad[1], None, None, None) == -1
        assert _lib.lib().serl_rb_import_slots(other.handle, bad[0], bad[1], None, None, None) == -1
    after = other.gather(idx)
    torch.cuda.synchronize()
    assert state == (len(other), other.latest_data_id(), other.insert_count(), other.rng_state())
    assert (mask == other.valid_mask()).all()
    for k in g2["keys"]:
        assert torch.equal(before["observations"][k], after["observations"][k])
    assert _np(before["rewards"]).tobytes() == _np(after["rewards"]).tobytes()


def test_damaged_snapshot_is_refused_and_the_store_untouched(gpu, tmp_path):
    g = GEOMS["two_cam"]
    a = _mk(g)
    a.seed(1)
    for tr in itertools.islice(_stream(g, 15), 60):
        a.insert(tr)
    m = a.save_snapshot(str(tmp_path / "snap"))
    fn = os.path.join(str(tmp_path / "snap"), m["segments"][0]["file"])
    raw = bytearray(open(fn, "rb").read())
    raw[1000] ^= 1
    open(fn, "wb").write(bytes(raw))
    for tr in itertools.islice(_stream(g, 15, seed=8), 20):
        a.insert(tr)
    idx = a.sample_indices(B)
    before, count = a.gather(idx), a.insert_count()
    with pytest.raises(ValueError, match=m["segments"][0]["file"]):
        a.restore_snapshot(str(tmp_path / "snap"))
    after = a.gather(idx)
    torch.cuda.synchronize()
    assert count == a.insert_count()
    for k in g["keys"]:
        assert torch.equal(before["observations"][k], after["observations"][k])


def test_unseeded_store_snapshot_carries_a_generator_state(gpu, tmp_path):
    g = GEOMS["one_cam"]
    a = _mk(g)
    for tr in itertools.islice(_stream(g, 15), 20):
        a.insert(tr)
    m = a.save_snapshot(str(tmp_path / "snap"))           # never seeded, never sampled: the lazy OS-entropy seed is drawn now
    assert int(m["rng"]["inc"]) != 0 and m["seed"] is not None
    b = _restored(g, str(tmp_path / "snap"))
    assert (a.sample_indices(64) == b.sample_indices(64)).all()   # (restoring must not draw a fresh seed over the snapshot's)


# ---- save under a concurrent inserter
class _CountingOracle(ReplayOracle):
    """the oracle's bookkeeping with its slot writes counted (frames of one byte: only the bookkeeping is used)"""
    writes = 0

    def _raw_insert(self, *a, **k):
        self.writes += 1
        return super()._raw_insert(*a, **k)


def _serial_transition(g, s):
    obs = {"state": np.full((1, g["S"]), s, np.float32)}
    nobs = {"state": np.full((1, g["S"]), s + 0.5, np.float32)}
    for k in g["keys"]:
        obs[k] = np.full((1, g["H"], g["W"], g["C"]), (s - 1) % 251, np.uint8)   # == the previous transition's next frame
        nobs[k] = np.full((1, g["H"], g["W"], g["C"]), s % 251, np.uint8)
    return {"observations": obs, "next_observations": nobs, "actions": np.zeros(g["A"], np.float32), "rewards": np.float32(s),
            "masks": np.float32(1), "dones": False}


def _check_serials(g, path):
    """The restored snapshot is a store between two inserts: its bookkeeping is the oracle's after the k transitions that
    make the manifest's count, every valid slot's record and frames carry one serial, and the valid slots hold exactly the last
    serials before k."""
    from serl_amd.data import snapshot as snap
    m = snap.read_manifest(path)
    o = _CountingOracle(g["keys"], 1, 1, 1, 1, g["S"], g["A"], g["cap"])
    tiny = dict(g, H=1, W=1, C=1)
    k = 0
    while o.writes < m["count"]:
        o.insert(_serial_transition(tiny, k))
        k += 1
    assert o.writes == m["count"], f"snapshot at slot write {m['count']}: inside transition {k - 1}'s insert"
    r = _restored(g, path)
    valid = r.valid_mask()
    assert len(r) == len(o) and r.latest_data_id() == o.insert_index and (valid == o.valid).all()
    idx = np.flatnonzero(valid).astype(np.int64)
    if len(idx) == 0:
        return k
    got = r.gather(idx.copy())
    torch.cuda.synchronize()
    serial = _np(got["rewards"])
    assert (serial == o.rewards[idx]).all()
    assert sorted(serial.astype(int)) == list(range(k - len(idx), k))
    assert (_np(got["observations"]["state"])[:, 0, 0] == serial).all()
    for key in g["keys"]:
        fr = _np(got["observations"][key])                 # [n][2][H][W][C]: the observation's frame and the next one
        want = (serial.astype(int) % 251).astype(np.uint8)
        assert (fr[:, 1] == want[:, None, None, None]).all()
        assert (fr[:, 0] == ((serial.astype(int) - 1) % 251).astype(np.uint8)[:, None, None, None]).all()
    return k


def test_save_under_a_concurrent_inserter(gpu, tmp_path):
    g = GEOMS["two_cam"]
    a = _mk(g)
    a.seed(0)
    N, marks = 200, (40, 100, 160)
    reached, go = [threading.Event() for _ in marks], [threading.Event() for _ in marks]
    errors = []

    def inserter():
        # at each mark the inserter waits for the main thread to be at the point of saving, then inserts on: every save STARTS
        # while inserts are running, and the first two cannot see the finished sequence (the inserter stops at the next mark)
        try:
            for s in range(N):
                a.insert(_serial_transition(g, s))
                for ev, ok, mk in zip(reached, go, marks):
                    if s == mk:
                        ev.set()
                        assert ok.wait(60), "the main thread never started its save"
        except BaseException as e:   # noqa: BLE001
            errors.append(e)
            for ev in reached:
                ev.set()

    t = threading.Thread(target=inserter, daemon=True)
    t.start()
    ks = []
    path = str(tmp_path / "snap")
    for i, ev in enumerate(reached):         # three snapshots while the inserter runs on: a full one, then two incremental
        assert ev.wait(60), "the inserter thread made no progress"
        assert not errors, errors
        go[i].set()
        a.save_snapshot(path, incremental=i > 0)
        ks.append(_check_serials(g, path))
    t.join(60)
    assert not t.is_alive(), "the inserter thread did not finish (an insert is stuck behind a snapshot)"
    assert not errors, errors
    assert all(k > mk for k, mk in zip(ks, marks)) and ks == sorted(ks) and ks[-1] <= N
    assert ks[0] <= marks[1] + 1 and ks[1] <= marks[2] + 1 and min(ks) < N     # snapshots of a store that was still being filled
    a.save_snapshot(path, incremental=True)
    assert _check_serials(g, path) == N


def test_export_slots_alone_holds_inserts_off(gpu):
    """The library's own guarantee, without the Python store's lock: while serl_rb_export_slots copies, inserts from another
    thread wait inside serl_rb_insert, so the mask and the slots it returns are of one instant -- every valid slot's record and
    frames carry one serial, and the valid slots hold exactly the last serials before some transition k."""
    import ctypes as C
    from serl_amd import _lib
    g = GEOMS["two_cam"]
    cap, rec_len = g["cap"], 2 * g["S"] + g["A"] + 3
    a = _mk(g)
    N, marks, errors = 300, (60, 180), []
    reached, go = [threading.Event() for _ in marks], [threading.Event() for _ in marks]

    def inserter():
        # waits at each mark until the main thread is at the point of exporting, then inserts on: the exports start while inserts
        # are running, and those of the first round cannot see the finished sequence (the inserter stops at the second mark)
        try:
            for s in range(N):
                a.insert(_serial_transition(g, s))
                for ev, ok, mk in zip(reached, go, marks):
                    if s == mk:
                        ev.set()
                        assert ok.wait(60), "the main thread never started its export"
        except BaseException as e:   # noqa: BLE001
            errors.append(e)
            for ev in reached:
                ev.set()

    t = threading.Thread(target=inserter, daemon=True)
    t.start()
    frames = [np.empty((cap, g["H"], g["W"], g["C"]), np.uint8) for _ in g["keys"]]
    rec, valid = np.empty((cap, rec_len), np.float32), np.empty(cap, np.uint8)
    fp = (C.c_void_p * len(frames))(*[f.ctypes.data for f in frames])
    seen = []
    for i, begin in enumerate((0, 17, 40, 5, 47)):          # the ring range starts anywhere and runs over the end
        if i in (0, 2):
            assert reached[i // 2].wait(60) and not errors, errors
            go[i // 2].set()
        _lib.check(_lib.lib().serl_rb_export_slots(a.handle, begin, cap, fp, rec.ctypes.data, valid.ctypes.data))
        slots = (begin + np.arange(cap)) % cap
        v = valid[slots].astype(bool)
        serial = rec[v, 2 * g["S"] + g["A"]].astype(int)            # the reward field
        assert (rec[v, 0] == serial).all()                          # state[0]
        for f in frames:
            assert (f[v] == (serial % 251).astype(np.uint8)[:, None, None, None]).all()
        k = serial.max() + 1
        assert sorted(serial) == list(range(k - len(serial), k)) and len(serial) >= cap - 3
        seen.append(k)
    t.join(60)
    assert not t.is_alive() and not errors, errors
    assert seen == sorted(seen) and a.insert_count() >= N
    assert marks[0] < seen[0] <= seen[1] <= marks[1] + 1 < N          # exports of a store that was still being filled
