"""GPU: a resumed learner run IS the uninterrupted run (serl_amd/utils/checkpoint.py save_run / restore_run).

Run A does 2K iterations of the loop of examples/learner_drq_synthetic.py (sample from the online and the demo store,
concat_batches, update_high_utd(utd_ratio=2), one insert per iteration).  Run B does K, calls save_run, destroys agent and
stores, builds fresh ones, calls restore_run and does K more.  Everything integer -- the indices sampled and the crop offsets
drawn in every iteration after the break, state.rng, step, the stores' generator and valid mask -- must be exactly equal.

Parameters and Adam moments: A is first run twice (that is code from before run resume existed).  Where A is bit-identical to
itself, B must be bit-identical to A; where it is not (fp32 atomics in the trunk statistics reorder sums between runs), B must
be within 2 x the largest elementwise |A - A'| of the same section (params, target_params, first moments, second moments): one
further, independent reordering.

A-versus-A figure: not yet measured.  The test prints both figures (A versus A, B versus A, per section) before it asserts;
they are to be recorded here and in DESIGN.md section 9."""
import gc
import itertools

import numpy as np
import pytest
import torch

from helpers import make_spaces

pytestmark = pytest.mark.gpu
KEYS, H, W, S, A, B, K, CAP = ("front", "wrist"), 64, 64, 7, 4, 8, 6, 64
SECTIONS = ("params", "target_params") + tuple(f"opt/{tx}/{m}" for tx in ("actor", "critic", "temperature") for m in ("mu", "nu"))
GROUP = {s: ("mu" if s.endswith("/mu") else "nu" if s.endswith("/nu") else s) for s in SECTIONS}


class _Box:
    def __init__(self, shape):
        self.shape = shape


class _Drq:
    """the pixel run: DrQ agent at 64x64, 2 cameras, reference parameter init; memory-efficient stores"""
    names = ("online", "demo")

    @staticmethod
    def agent(seed=42):
        from serl_amd.utils.launcher import make_drq_agent
        obs = {k: np.zeros((1, H, W, 3), np.uint8) for k in KEYS}
        obs["state"] = np.zeros((1, S), np.float32)
        return make_drq_agent(seed, obs, np.zeros((A,), np.float32), image_keys=KEYS, encoder_type="resnet-pretrained",
                              batch_size=B, param_init="reference")

    @staticmethod
    def store():
        from serl_amd.data.data_store import MemoryEfficientReplayBufferDataStore
        osp, asp = make_spaces(KEYS, H, W, 3, 1, S, A)
        return MemoryEfficientReplayBufferDataStore(osp, asp, CAP, image_keys=KEYS)

    @staticmethod
    def stream(seed):
        from serl_amd.utils.synthetic import transition_stream
        return transition_stream(KEYS, H, W, 3, 1, S, A, 9, seed)


class _Sac:
    """the state-only run: make_sac_agent + ReplayBufferDataStore"""
    names = ("online", "demo")

    @staticmethod
    def agent(seed=42):
        from serl_amd.utils.launcher import make_sac_agent
        return make_sac_agent(seed, np.zeros((S,), np.float32), np.zeros((A,), np.float32), batch_size=B, param_init="reference")

    @staticmethod
    def store():
        from serl_amd.data.data_store import ReplayBufferDataStore
        return ReplayBufferDataStore(_Box((S,)), _Box((A,)), capacity=CAP)

    @staticmethod
    def stream(seed):
        from serl_amd.utils.synthetic import flat_stream
        return flat_stream(S, A, 9, seed)


def _build(kind):
    """agent + {name: store}, each store seeded and holding 40 transitions; the online store wraps during the run"""
    agent = kind.agent()
    stores = {}
    for i, name in enumerate(kind.names):
        st = kind.store()
        st.seed(100 + i)
        for tr in itertools.islice(kind.stream(7 + i), 40 if name == "demo" else CAP - 5):
            st.insert(tr)
        stores[name] = st
    return agent, stores


def _iterate(agent, stores, feed, n, log):
    from serl_amd.data.data_store import concat_batches
    for _ in range(n):
        batch = concat_batches(stores["online"].sample(B // 2, lazy=True), stores["demo"].sample(B // 2, lazy=True), axis=0)
        agent, info = agent.update_high_utd(batch, utd_ratio=2)
        stores["online"].insert(next(feed))
        rec = {"idx": [ix.copy() for _, ix in batch.parts], "rng": np.array(agent.state.rng), "step": int(agent.state.step)}
        for k in ("crop_obs", "crop_next"):
            if k in agent.last_draws:
                rec[k] = np.array(agent.last_draws[k])
        log.append(rec)
    return agent


def _final(agent, stores):
    torch.cuda.synchronize()
    core = agent.core
    leaves = [n for n in core.leaves if not n.startswith("trunk/")]      # the trunk is frozen
    out = {"rng": np.array(agent.state.rng), "step": int(agent.state.step),
           "stores": {n: (len(s), s.latest_data_id(), s.insert_count(), s.rng_state(), s.valid_mask()) for n, s in stores.items()},
           "theta": {(sec, n): core.get(sec, n).copy() for sec in SECTIONS for n in leaves}}
    return out


def _run_a(kind):
    agent, stores = _build(kind)
    feed, log = kind.stream(99), []
    agent = _iterate(agent, stores, feed, 2 * K, log)
    return log, _final(agent, stores)


def _run_b(kind, run_dir):
    from serl_amd.utils.checkpoint import restore_checkpoint, restore_run, save_run
    agent, stores = _build(kind)
    feed, log = kind.stream(99), []
    agent = _iterate(agent, stores, feed, K, log)
    saved_rng, saved_step = np.array(agent.state.rng), int(agent.state.step)
    save_run(run_dir, agent, stores, step=saved_step)
    del agent, stores
    gc.collect()
    torch.cuda.synchronize()
    # a fresh process would start here: other seeds than the original's show that nothing survives but the files
    agent = kind.agent(seed=7)
    stores = {n: kind.store() for n in kind.names}
    fresh_rng = np.array(agent.state.rng)
    assert not np.array_equal(fresh_rng, saved_rng)
    restore_checkpoint(run_dir, agent)                       # the default: everything but the rng, as before
    assert np.array_equal(agent.state.rng, fresh_rng) and int(agent.state.step) == saved_step
    assert restore_run(run_dir, agent, stores) == saved_step
    assert np.array_equal(agent.state.rng, saved_rng) and int(agent.state.step) == saved_step
    agent = _iterate(agent, stores, feed, K, log)
    return log, _final(agent, stores)


def _same_integers(x, y):
    (lx, fx), (ly, fy) = x, y
    assert len(lx) == len(ly) == 2 * K
    for i, (p, q) in enumerate(zip(lx, ly)):
        assert sorted(p) == sorted(q), i
        assert all(np.array_equal(a, b) for a, b in zip(p["idx"], q["idx"])), f"iteration {i}: sampled indices differ"
        for k in ("rng", "crop_obs", "crop_next"):
            assert k not in p or np.array_equal(p[k], q[k]), f"iteration {i}: {k} differs"
        assert p["step"] == q["step"], i
    assert np.array_equal(fx["rng"], fy["rng"]) and fx["step"] == fy["step"]
    for n in fx["stores"]:
        for u, v in zip(fx["stores"][n][:4], fy["stores"][n][:4]):
            assert u == v, n
        assert np.array_equal(fx["stores"][n][4], fy["stores"][n][4]), n


def _max_diff(fx, fy):
    d = {g: 0.0 for g in GROUP.values()}
    for key, v in fx["theta"].items():
        w = fy["theta"][key]
        if v.tobytes() != w.tobytes():
            assert np.isfinite(v).all() and np.isfinite(w).all(), key
            d[GROUP[key[0]]] = max(d[GROUP[key[0]]], float(np.abs(v.astype(np.float64) - w).max()), np.finfo(np.float32).tiny)
    return d


@pytest.mark.parametrize("kind", [_Drq, _Sac], ids=["drq_pixels", "sac_state"])
def test_resumed_run_is_the_uninterrupted_run(gpu, tmp_path, kind):
    a1 = _run_a(kind)
    a2 = _run_a(kind)
    _same_integers(a1, a2)
    noise = _max_diff(a1[1], a2[1])                      # A versus A: the parent's own run-to-run difference
    print("A-versus-A largest elementwise difference per section:", noise)
    b = _run_b(kind, str(tmp_path / "run"))
    _same_integers(a1, b)
    got = _max_diff(a1[1], b[1])
    print("B-versus-A largest elementwise difference per section:", got)
    assert a1[1]["step"] == 2 * K * 3
    for g in noise:
        assert got[g] <= 2 * noise[g], f"{g}: resumed run differs from the uninterrupted one by {got[g]}, A-versus-A by {noise[g]}"


def test_save_run_keeps_and_prunes_steps_and_saves_incrementally(gpu, tmp_path):
    import os
    from serl_amd.data import snapshot as snap
    from serl_amd.data.data_store import ReplayBufferDataStore
    from serl_amd.utils.checkpoint import restore_run, save_run
    kind, run_dir = _Sac, str(tmp_path / "run")
    agent, stores = _build(kind)
    feed = kind.stream(5)
    for step in (10, 20, 30):
        for _ in range(6):
            stores["online"].insert(next(feed))
        save_run(run_dir, agent, stores, step=step, keep=2)
    assert sorted(os.listdir(run_dir)) == sorted(["checkpoint_20", "checkpoint_30"] + [f"store_{n}_{s}" for n in kind.names for s in (20, 30)])
    m = snap.read_manifest(os.path.join(run_dir, "store_online_30"))
    assert [s["n_slots"] for s in m["segments"]][-2:] == [6, 6]          # only the slots written since the previous step
    assert snap.read_manifest(os.path.join(run_dir, "store_demo_30"))["segments"][-1]["n_slots"] == 40
    snap.verify_snapshot(os.path.join(run_dir, "store_online_30"), m)    # step 10's directory is gone, its files live on here
    fresh = {n: kind.store() for n in kind.names}
    assert restore_run(run_dir, agent, fresh, step=20) == 20
    assert fresh["online"].insert_count() == stores["online"].insert_count() - 6
    assert restore_run(run_dir, agent, fresh) == 30
    assert fresh["online"].insert_count() == stores["online"].insert_count()
    with pytest.raises(FileNotFoundError):
        restore_run(str(tmp_path / "nothing"), agent, fresh)
    # a damaged store snapshot of an explicitly requested step, or stores of another geometry: refused before the agent or any
    # store is touched
    seg = os.path.join(run_dir, "store_demo_30", snap.read_manifest(os.path.join(run_dir, "store_demo_30"))["segments"][0]["file"])
    os.remove(seg)                                   # (the name is a hard link shared with step 20: replace it, do not truncate it)
    open(seg, "wb").write(b"x" * 100)
    other = kind.agent(seed=3)
    rng0, step0 = np.array(other.state.rng), int(other.state.step)
    with pytest.raises(ValueError, match="store_demo_30"):
        restore_run(run_dir, other, {n: kind.store() for n in kind.names}, step=30)
    bigger = {"online": kind.store(), "demo": ReplayBufferDataStore(_Box((S,)), _Box((A,)), capacity=CAP + 1)}
    with pytest.raises(ValueError, match="store_demo_20"):
        restore_run(run_dir, other, bigger, step=20)
    assert np.array_equal(other.state.rng, rng0) and int(other.state.step) == step0 and len(bigger["online"]) == 0
    # without a step: the newest complete step whose stores all check
    assert restore_run(run_dir, other, fresh) == 20
    assert int(other.state.step) == int(agent.state.step) and fresh["online"].insert_count() == stores["online"].insert_count() - 6


def _store_rings(stores, tmp_path, tag):
    """every live slot, the mask and the bookkeeping of each store, through a full snapshot of it"""
    from serl_amd.data import snapshot as snap
    out = {}
    for n, st in stores.items():
        p = str(tmp_path / f"ring_{tag}_{n}")
        st.save_snapshot(p)
        m, valid, segs = snap.read_snapshot(p)
        r = snap.assemble(m, valid, segs)
        w = r["written"]
        out[n] = (m["size"], m["insert_index"], m["count"], m["first"], m["rng"], r["valid"].tobytes(), w.tobytes(),
                  r["records"][w].tobytes(), [f[w].tobytes() for f in r["frames"]])
    return out


@pytest.mark.parametrize("kind", [_Sac, _Drq], ids=["sac_state", "drq_pixels"])
def test_a_save_that_died_is_never_extended(gpu, tmp_path, kind):
    """Step 10 is saved; the save of step 20 writes its stores and dies before the checkpoint file.  The resumed process
    continues from step 10 with OTHER transitions: its save at step 30 must not build on step 20's orphaned snapshots (their
    counts and geometry fit, their slots are another history's)."""
    import os
    from serl_amd.utils.checkpoint import restore_run, save_run
    run_dir = str(tmp_path / "run")
    agent, stores = _build(kind)
    feed = kind.stream(5)
    save_run(run_dir, agent, stores, step=10, keep=3)
    for _ in range(8):
        stores["online"].insert(next(feed))
    save_run(run_dir, agent, stores, step=20, keep=3)
    os.remove(os.path.join(run_dir, "checkpoint_20"))                 # ... as if the process had died just before writing it
    del stores
    gc.collect()
    stores = {n: kind.store() for n in kind.names}
    assert restore_run(run_dir, agent, stores) == 10
    other = kind.stream(1234)
    for _ in range(12):                                               # a different history, 12 > 8 slot writes past step 10
        stores["online"].insert(next(other))
    save_run(run_dir, agent, stores, step=30, keep=3)
    assert not os.path.exists(os.path.join(run_dir, "store_online_20")) and not os.path.exists(os.path.join(run_dir, "store_demo_20"))
    again = {n: kind.store() for n in kind.names}
    assert restore_run(run_dir, agent, again) == 30
    assert _store_rings(again, tmp_path, "restored") == _store_rings(stores, tmp_path, "live")
    # saving a complete step again replaces it whole
    stores["online"].insert(next(other))
    save_run(run_dir, agent, stores, step=30, keep=3)
    assert restore_run(run_dir, agent, again) == 30
    assert _store_rings(again, tmp_path, "restored2") == _store_rings(stores, tmp_path, "live2")
    assert not [n for n in os.listdir(run_dir) if n.endswith(".tmp")]
