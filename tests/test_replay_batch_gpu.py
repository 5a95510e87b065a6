"""GPU: batch_insert of the HBM replay stores (serl_rb_insert_batch: one host-to-device copy and one insert_scatter_kernel launch
per staging slot of slot writes) must leave, byte for byte, what insert() per transition leaves -- frames, records, valid mask,
size, insert_index, insert_count and first -- and not touch the sampler's generator.  Integer / byte work: every comparison is
exact."""
import ctypes as C
import pickle
import threading

import numpy as np
import pytest
import torch

from helpers import make_spaces
from oracle.replay_oracle import PlainReplayOracle, ReplayOracle

pytestmark = pytest.mark.gpu

GEOMS = {
    "a": dict(keys=("front", "wrist"), T=1, H=8, W=16, S=5, A=3, cap=37),
    "b": dict(keys=("image",), T=2, H=5, W=16, S=4, A=2, cap=23),
    "c": dict(keys=("image",), T=4, H=4, W=16, S=3, A=2, cap=19),
    "d": dict(keys=(), T=1, H=0, W=0, S=6, A=2, cap=16),            # ReplayBufferDataStore: flat observations, no frames
    "e": dict(keys=("front", "wrist"), T=1, H=128, W=128, S=7, A=4, cap=24),
}


def _mk(g, cap=None):
    from serl_amd.data.data_store import MemoryEfficientReplayBufferDataStore, ReplayBufferDataStore
    from helpers import _Sp
    cap = cap or g["cap"]
    if not g["keys"]:
        return ReplayBufferDataStore(_Sp((g["S"],)), _Sp((g["A"],)), cap)
    osp, asp = make_spaces(g["keys"], g["H"], g["W"], 3, g["T"], g["S"], g["A"])
    return MemoryEfficientReplayBufferDataStore(osp, asp, cap, image_keys=g["keys"])


def _oracle(g):
    if not g["keys"]:
        return PlainReplayOracle(g["S"], g["A"], g["cap"])
    return ReplayOracle(g["keys"], g["H"], g["W"], 3, g["T"], g["S"], g["A"], g["cap"])


def _stream(g, n, seed=3, p_done=0.2):
    """n seeded transitions, each `done` with probability p_done, every frame and field random"""
    rng = np.random.default_rng(seed)
    T, S = g["T"], g["S"]
    out = []
    for _ in range(n):
        done = bool(rng.random() < p_done)
        if g["keys"]:
            obs, nobs = ({"state": rng.standard_normal((T, S)).astype(np.float32),
                          **{k: rng.integers(0, 256, (T, g["H"], g["W"], 3), dtype=np.uint8) for k in g["keys"]}} for _ in range(2))
        else:
            obs, nobs = (rng.standard_normal(S).astype(np.float32) for _ in range(2))
        out.append({"observations": obs, "next_observations": nobs, "actions": rng.standard_normal(g["A"]).astype(np.float32),
                    "rewards": np.float32(rng.standard_normal()), "masks": np.float32(1.0 - done), "dones": done})
    return out


def _payloads(g, transitions, sizes=None):
    """the stream cut into payloads whose sizes cycle 1, 2, 7, cap-1, cap, 2*cap+3"""
    cap = g["cap"]
    sizes = sizes or [1, 2, 7, cap - 1, cap, 2 * cap + 3]
    at, k = 0, 0
    while at < len(transitions):
        yield transitions[at:at + sizes[k % len(sizes)]]
        at += sizes[k % len(sizes)]
        k += 1


def _state(store):
    from serl_amd.data.data_store import _meta_state
    return _meta_state(store._meta())   # size, insert_index, count, first, rng


def _export(store):
    """-> (frames per camera, records) of the slots [0, size), as serl_rb_export_slots gives them"""
    from serl_amd import _lib
    m = store._meta()
    cap, n_cam = int(m.capacity), len(store.pixel_keys)
    frames = [np.zeros((cap, m.H, m.W, m.C), np.uint8) for _ in range(n_cam)]
    records = np.zeros((cap, m.rec_len), np.float32)
    fp = (C.c_void_p * max(n_cam, 1))(*[f.ctypes.data for f in frames])
    _lib.check(_lib.lib().serl_rb_export_slots(store.handle, 0, cap, fp if n_cam else None, records.ctypes.data, None))
    n = len(store)
    return [f[:n] for f in frames], records[:n]


def _assert_same_contents(a, b):
    assert _state(a) == _state(b)
    assert (a.valid_mask() == b.valid_mask()).all()
    (fa, ra), (fb, rb) = _export(a), _export(b)
    for x, y in zip(fa, fb):
        assert x.tobytes() == y.tobytes(), "frames differ"
    assert ra.tobytes() == rb.tobytes(), "records differ"


def _flat(d, prefix=""):
    for k, v in d.items():
        if isinstance(v, dict):
            yield from _flat(v, prefix + k + ".")
        else:
            yield prefix + k, v


@pytest.mark.parametrize("name", sorted(GEOMS))
def test_batch_insert_equals_per_transition_inserts(gpu, name):
    g = GEOMS[name]
    cap = g["cap"]
    a, b, o = _mk(g), _mk(g), _oracle(g)
    a.seed(9)
    b.seed(9)
    rng0 = _state(b)["rng"]
    transitions = _stream(g, 3 * cap + 5)
    crossed_wrap = own_slots = 0
    for payload in _payloads(g, transitions, [20] if name == "e" else None):
        before = b.insert_count()
        for tr in payload:
            a.insert(tr)
            o.insert(tr)
        b.batch_insert(payload)
        crossed_wrap += before // cap != b.insert_count() // cap
        own_slots += b.insert_count() - before > cap
        sa, sb = _state(a), _state(b)
        assert sa == sb and sb["rng"] == rng0, (sa, sb)
        assert sb["size"] == len(o) == len(b) and sb["insert_index"] == o.insert_index
        va, vb = a.valid_mask(), b.valid_mask()
        assert (va == vb).all()
        if g["keys"]:
            assert sb["first"] == o.first and (vb == o.valid).all()
        else:
            assert vb[:len(o)].all() and not vb[len(o):].any()
    # payloads cross the wrap; with frames, a payload of cap transitions writes more than cap slots: it overwrites its own
    assert crossed_wrap >= 2 and (name in "de" or own_slots >= 1)
    assert b.insert_stats()["batch_calls"] >= 4 and a.insert_stats()["batch_calls"] == 0
    _assert_same_contents(a, b)
    a.seed(5)
    b.seed(5)
    o.seed(5)
    for _ in range(3):
        ia, ib = a.sample_indices(16), b.sample_indices(16)
        assert (ia == ib).all() and (ib == o.sample_indices(16)).all()
        ga, gb = dict(_flat(a.gather(ia))), dict(_flat(b.gather(ib)))
        torch.cuda.synchronize()
        assert sorted(ga) == sorted(gb)
        for k in ga:
            assert ga[k].cpu().numpy().tobytes() == gb[k].cpu().numpy().tobytes(), k
        go = dict(_flat(o.gather(ib)))
        for k in go:   # and they are the oracle's
            assert (gb[k].cpu().numpy() == go[k]).all(), k


def test_a_payload_is_one_call_one_copy_one_launch(gpu):
    g = GEOMS["a"]
    b = _mk(g, cap=64)
    transitions = _stream(g, 20, p_done=0.1)
    s0 = b.insert_stats()
    assert s0 == dict(transitions=0, batch_calls=0, h2d_copies=0, launches=0)
    b.batch_insert(transitions[:10])          # no wrap (at most 20 slot writes of 64), far below the staging budget
    s1 = b.insert_stats()
    assert s1 == dict(transitions=10, batch_calls=1, h2d_copies=1, launches=1)
    writes = b.insert_count()
    for tr in transitions[10:]:
        b.insert(tr)
    s2 = b.insert_stats()
    assert s2["batch_calls"] == 1 and s2["launches"] == 1 and s2["transitions"] == 20
    assert s2["h2d_copies"] == 1 + (b.insert_count() - writes) * (len(g["keys"]) + 1)   # n_cam + 1 copies per slot write
    a = _mk(g, cap=64)
    for tr in transitions:
        a.insert(tr)
    _assert_same_contents(a, b)


@pytest.mark.parametrize("name", ["a", "c", "d"])
def test_a_payload_longer_than_the_ring(gpu, name):
    g = GEOMS[name]
    transitions = _stream(g, 5 + 2 * g["cap"] + 3, seed=8)
    a, b = _mk(g), _mk(g)
    for tr in transitions:
        a.insert(tr)
    b.batch_insert(transitions[:5])
    b.batch_insert(transitions[5:])            # 2 * cap + 3 transitions in one call
    s = b.insert_stats()
    assert s["batch_calls"] == 2 and s["launches"] >= 4 and s["launches"] == s["h2d_copies"]
    _assert_same_contents(a, b)


def _c_arrays(g, transitions):
    """the arguments of serl_rb_insert_batch for `transitions` (and what keeps them alive)"""
    n, n_cam = len(transitions), len(g["keys"])
    fo = [np.ascontiguousarray(tr["observations"][k]) for tr in transitions for k in g["keys"]]
    fn = [np.ascontiguousarray(tr["next_observations"][k]) for tr in transitions for k in g["keys"]]
    obs_p = (C.c_void_p * (n * n_cam))(*[x.ctypes.data for x in fo])
    next_p = (C.c_void_p * (n * n_cam))(*[x.ctypes.data for x in fn])
    st = np.stack([tr["observations"]["state"].reshape(-1) for tr in transitions])
    nst = np.stack([tr["next_observations"]["state"].reshape(-1) for tr in transitions])
    act = np.stack([tr["actions"] for tr in transitions])
    rew = np.array([tr["rewards"] for tr in transitions], np.float32)
    msk = np.array([tr["masks"] for tr in transitions], np.float32)
    done = np.array([tr["dones"] for tr in transitions], np.uint8)
    keep = (fo, fn, st, nst, act, rew, msk, done)
    return obs_p, next_p, [x.ctypes.data for x in (st, nst, act, rew, msk, done)], keep


def test_refused_calls_leave_the_store_untouched(gpu):
    from serl_amd import _lib
    g = GEOMS["a"]
    b = _mk(g)
    transitions = _stream(g, 16)
    b.batch_insert(transitions[:6])
    before = (len(b), _state(b), b.valid_mask(), b.insert_stats())

    def untouched():
        return len(b) == before[0] and _state(b) == before[1] and (b.valid_mask() == before[2]).all() and b.insert_stats() == before[3]

    L = _lib.lib()
    obs_p, next_p, small, keep = _c_arrays(g, transitions[6:])
    n = len(transitions) - 6
    for table, k in ((obs_p, 2 * 4 + 1), (next_p, 2 * 7)):     # a NULL entry at position k of either table
        saved, table[k] = table[k], None
        assert L.serl_rb_insert_batch(b.handle, n, obs_p, next_p, *small) != 0 and b"NULL" in L.serl_last_error()
        table[k] = saved
        assert untouched()
    assert L.serl_rb_insert_batch(b.handle, -1, obs_p, next_p, *small) != 0 and untouched()
    assert L.serl_rb_insert_batch(b.handle, n, None, next_p, *small) != 0 and untouched()
    assert L.serl_rb_insert_batch(b.handle, n, obs_p, next_p, *small[:5], None) != 0 and untouched()
    assert L.serl_rb_insert_batch(b.handle, 0, None, None, None, None, None, None, None, None) == 0 and untouched()
    # a Python payload whose fifth transition has a wrong frame shape raises before anything is inserted
    bad = [dict(tr) for tr in transitions[6:]]
    bad[4]["observations"] = dict(bad[4]["observations"], front=np.zeros((1, 8, 32, 3), np.uint8))
    with pytest.raises(AssertionError):
        b.batch_insert(bad)
    assert untouched()
    b.batch_insert([])
    assert untouched()
    # the same arguments, whole, are accepted -- and are what batch_insert passes
    assert L.serl_rb_insert_batch(b.handle, n, obs_p, next_p, *small) == 0
    a = _mk(g)
    a.batch_insert(transitions[:6])
    a.batch_insert(transitions[6:])
    _assert_same_contents(a, b)


# ---- threads: frames, state and reward encode the transition's number
TG = dict(keys=("front", "wrist"), T=1, H=16, W=16, S=4, A=2, cap=150)
EP = 13


def _frame(k, cam):
    base = (int(k) * 97 + cam * 31) % 251
    return ((np.arange(16 * 16 * 3, dtype=np.int64) * 7 + base) % 256).astype(np.uint8).reshape(1, 16, 16, 3)


def _numbered(k):
    """transition k: obs frame k, next frame k + 1 (consecutive steps of an episode share a frame)"""
    done = (k % EP) == EP - 1
    st = np.full((1, TG["S"]), k, np.float32)
    obs = {"state": st, **{c: _frame(k, i) for i, c in enumerate(TG["keys"])}}
    nobs = {"state": st + 0.5, **{c: _frame(k + 1, i) for i, c in enumerate(TG["keys"])}}
    return {"observations": obs, "next_observations": nobs, "actions": np.full(TG["A"], k, np.float32), "rewards": np.float32(k),
            "masks": np.float32(1.0 - done), "dones": bool(done)}


def test_batch_insert_thread_against_gathers(gpu):
    from serl_amd.agents.batch import DeviceBatch
    from serl_amd.data.data_store import gather_crop
    B, g = 16, TG
    rb = _mk(g)
    rb.seed(0)
    rb.batch_insert([_numbered(k) for k in range(48)])
    err, inserted = [], [48]

    def inserter():      # 40 payloads of 16, however fast the main thread runs: the ring of 150 wraps four times
        try:
            for _ in range(40):
                rb.batch_insert([_numbered(k) for k in range(inserted[0], inserted[0] + 16)])
                inserted[0] += 16
        except Exception as e:  # noqa: BLE001
            err.append(e)

    th = threading.Thread(target=inserter)
    out = DeviceBatch(B, 2, g["H"], g["W"], 3, g["S"], g["A"], 0)
    th.start()
    checked = iters = 0
    while iters < 30 or (th.is_alive() and iters < 400):     # 30 iterations, and on for as long as the inserter runs
        iters += 1
        idx = rb.sample_indices(B)
        gather_crop([(rb, idx)], None, None, out)     # (stale indices are re-drawn in place: `idx` describes the batch)
        torch.cuda.synchronize()
        frames, state, reward = out.frames.cpu().numpy(), out.state.cpu().numpy(), out.reward.cpu().numpy()
        for j in range(B):
            k = int(reward[j])
            assert (state[0, j] == k).all() and (state[1, j] == k + 0.5).all(), f"sample {j}: record of transition {k} is torn"
            if idx[j] == 0:      # the reference's negative window (tests/test_replay_threads_gpu.py): not the slot's own frames
                assert k % EP == 0
                continue
            for c in range(2):
                assert (frames[0, c, j] == _frame(k, c)[0]).all(), f"sample {j}: observation frame of transition {k}"
                assert (frames[1, c, j] == _frame(k + 1, c)[0]).all(), f"sample {j}: next frame of transition {k}"
            checked += 1
    th.join(timeout=60)
    assert not th.is_alive() and not err, err
    assert checked >= 25 * B and inserted[0] == 48 + 40 * 16, (checked, inserted[0])
    a = _mk(g)
    for k in range(inserted[0]):
        a.insert(_numbered(k))
    sa, sb = _state(a), _state(rb)
    assert {k: sa[k] for k in ("size", "insert_index", "count", "first")} == {k: sb[k] for k in ("size", "insert_index", "count", "first")}
    assert (a.valid_mask() == rb.valid_mask()).all()
    (fa, ra), (fb, rb_) = _export(a), _export(rb)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(fa, fb)) and ra.tobytes() == rb_.tobytes()
    print(f"batch_insert thread: {inserted[0] - 48} transitions, {iters} gather iterations, {checked} gathered samples verified")


def test_snapshot_after_batch_insert(gpu, tmp_path):
    g = GEOMS["a"]
    transitions = _stream(g, 70)
    a = _mk(g)
    a.seed(4)
    a.batch_insert(transitions[:45])           # 45 transitions: the ring of 37 has wrapped
    path = str(tmp_path / "snap")
    m = a.save_snapshot(path)
    assert m["count"] == a.insert_count() > g["cap"]
    b = _mk(g)
    b.restore_snapshot(path)
    _assert_same_contents(a, b)
    a.batch_insert(transitions[45:60])
    b.batch_insert(transitions[45:60])
    _assert_same_contents(a, b)
    m2 = a.save_snapshot(path, incremental=True)
    assert len(m2["segments"]) == len(m["segments"]) + 1
    c = _mk(g)
    c.restore_snapshot(path)
    _assert_same_contents(a, c)
    ref = _mk(g)
    for tr in transitions[:60]:
        ref.insert(tr)
    ref.seed(4)
    _assert_same_contents(ref, c)


def test_trainer_server_message_is_one_batched_call(gpu):
    from serl_amd.transport import QueuedDataStore, TrainerClient, TrainerServer, make_trainer_config
    g = GEOMS["a"]
    store, transitions = _mk(g), _stream(g, 12)
    cfg = make_trainer_config(port_number=6741, broadcast_port=6742)
    server = TrainerServer(cfg, transport="loopback")
    server.register_data_store("actor_env", store)
    server.start(threaded=True)
    try:
        local = QueuedDataStore(100)
        client = TrainerClient("actor_env", "localhost", cfg, local, wait_for_server=True, transport="loopback")
        for tr in transitions:
            local.insert(tr)
        assert client.update()
    finally:
        server.stop()
    s = store.insert_stats()
    assert s["transitions"] == 12 and s["batch_calls"] == 1 and s["launches"] == 1 and s["h2d_copies"] == 1
    a = _mk(g)
    for tr in transitions:
        a.insert(tr)
    _assert_same_contents(a, store)


def test_populate_data_store_batches(gpu, tmp_path, capsys):
    from serl_amd.data.data_store import populate_data_store
    g = GEOMS["b"]
    transitions = _stream(g, 40)
    path = str(tmp_path / "demos.pkl")
    with open(path, "wb") as f:
        pickle.dump(transitions, f)
    b = _mk(g, cap=128)
    assert populate_data_store(b, [path]) is b
    assert capsys.readouterr().out == f"Loaded {len(b)} transitions.\n"
    a = _mk(g, cap=128)
    for tr in transitions:
        a.insert(tr)
    _assert_same_contents(a, b)
    s = b.insert_stats()
    assert s["batch_calls"] >= 1 and s["transitions"] == 40
