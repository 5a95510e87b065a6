"""GPU: parameter snapshots (agent.snapshot(), csrc/snapshot.hip, serl_amd/agents/snapshot.py).  The shapes are the smallest at
which the pack kernel can go wrong: a state-only SAC agent with S = 3, A = 5, hidden 64, ensemble 3, B = 8 (five-float biases and the
one-float temp/lagrange make run lengths that are no multiple of four: the scalar tail runs), a frozen-trunk DrQ agent at 32x32 with
one camera, A = 1, B = 4 (the trunk's runs span many 16 KB parts) and a SmallEncoder agent at 32x32 with num_stack = 2, B = 4.
Everything is compared bit for bit against a twin agent (same seed, same resident batch, same draws) read through agent.state."""
import os
import queue
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ALL = ("params", "target_params", "opt_states")
MLP = {"hidden_dims": [64, 64], "activations": "tanh", "use_layer_norm": True}
TIMEOUT = 20.0


def _agent(kind, seed=3):
    from serl_amd.agents.drq import DrQAgent
    from serl_amd.agents.sac import SACAgent
    if kind == "sac":
        opt = {"learning_rate": 3e-4, "warmup_steps": 0}
        return SACAgent.create_states(seed, np.zeros((3,), np.float32), np.zeros((5,), np.float32), critic_ensemble_size=3,
                                      critic_subsample_size=2, critic_network_kwargs=MLP, policy_network_kwargs=dict(MLP),
                                      actor_optimizer_kwargs=opt, critic_optimizer_kwargs=opt, batch_size=8)
    T = 2 if kind == "small" else 1
    obs = {"image": np.zeros((T, 32, 32, 3), np.uint8), "state": np.zeros((T, 3), np.float32)}
    return DrQAgent.create_drq(seed, obs, np.zeros((1,), np.float32), encoder_type="small" if kind == "small" else "resnet-pretrained",
                               use_proprio=True, image_keys=("image",), critic_network_kwargs=MLP, policy_network_kwargs=dict(MLP),
                               critic_ensemble_size=3, critic_subsample_size=2, batch_size=4)


def _batch(agent, seed=11):
    """a resident device batch of the agent's full size, already cropped"""
    from serl_amd.agents.batch import DeviceBatch
    c = agent.core.cfg
    db = DeviceBatch(c.batch, c.n_cam, c.H, c.W, 3, c.state_dim, c.act_dim, 0, agent.num_stack)
    g = torch.Generator().manual_seed(seed)
    db.frames.copy_(torch.randint(0, 256, tuple(db.frames.shape), generator=g, dtype=torch.uint8))
    db.state.copy_(torch.randn(tuple(db.state.shape), generator=g))
    db.action.copy_(torch.rand(tuple(db.action.shape), generator=g) * 2 - 1)
    db.reward.copy_((torch.rand(tuple(db.reward.shape), generator=g) < 0.3).float())
    db.mask.copy_((torch.rand(tuple(db.mask.shape), generator=g) < 0.9).float())
    db.done.zero_()
    return db


def _step(agent, db, i):
    """update i of the schedule every test uses: actor + temperature move on the even ones"""
    if i % 2 == 0:
        if agent.image_keys:
            agent.update_high_utd(db, utd_ratio=1)
        else:
            agent.update(db)
    elif agent.image_keys:
        agent.update_critics(db)
    else:
        agent.update(db, networks_to_update=frozenset({"critic"}))


def _flat(tree, prefix=()):
    out = {}
    for k, v in tree.items():
        if isinstance(v, dict):
            out.update(_flat(v, prefix + (k,)))
        else:
            out[prefix + (k,)] = np.asarray(v)
    return out


def _assert_same_bits(got, want, what):
    g, w = _flat(got), _flat(want)
    assert list(g) == list(w), (what, "tree structure or key order differs")
    for k in g:
        assert g[k].shape == w[k].shape and g[k].dtype == w[k].dtype, (what, k, g[k].shape, w[k].shape, g[k].dtype, w[k].dtype)
        assert g[k].tobytes() == w[k].tobytes(), (what, k)


def _copy_tree(tree):
    return {k: _copy_tree(v) if isinstance(v, dict) else np.array(v) for k, v in tree.items()}


def _state_copy(state):
    return {"step": int(state.step), "rng": np.array(state.rng), "params": _copy_tree(state.params),
            "target_params": _copy_tree(state.target_params), "opt_states": _copy_tree(state.opt_states)}


@pytest.mark.parametrize("kind", ["sac", "frozen", "small"])
def test_snapshot_is_consistent_under_a_running_stream(gpu, kind):
    k = 2
    agent, twin = _agent(kind), _agent(kind)
    db = _batch(agent)
    for i in range(k):
        _step(agent, db, i)
        _step(twin, db, i)
    want = _state_copy(twin.state)
    snap = agent.snapshot(ALL)
    for i in range(k, k + 3):       # no synchronisation between the take and these
        _step(agent, db, i)
    snap.wait()
    assert snap.ready() and snap.finite and snap.nonfinite == {s: 0 for s in ALL}
    assert snap.step == want["step"] and np.array_equal(snap.rng, want["rng"])
    for name in ALL:
        _assert_same_bits(getattr(snap, name), want[name], name)
    leaf = _flat(snap.params)[("modules_critic", "network", "Dense_0", "kernel")]
    assert not leaf.flags.writeable and not leaf.flags.owndata           # a view into the pinned buffer, not a copy
    live = _flat(agent.state.params)
    moved = [p for p, v in _flat(snap.params).items() if p[0] == "modules_critic" and v.tobytes() != live[p].tobytes()]
    assert moved, "the live critic after three more updates equals the snapshot: a view of the arena, not a copy?"
    assert agent.state.step > snap.step
    snap.release()


def test_slots_are_held_until_released(gpu):
    from serl_amd._lib import SerlError
    agent = _agent("sac")
    db = _batch(agent)
    _step(agent, db, 0)
    s1 = agent.snapshot(("params",), slots=2)
    _step(agent, db, 1)
    s2 = agent.snapshot(("params",), slots=2)
    p1, p2 = _copy_tree(s1.params), _copy_tree(s2.params)
    assert _flat(p1)[("modules_critic", "network", "Dense_0", "kernel")].tobytes() != \
        _flat(p2)[("modules_critic", "network", "Dense_0", "kernel")].tobytes()
    _step(agent, db, 2)
    with pytest.raises(SerlError, match=r"status -3"):
        agent.snapshot(("params",), slots=2)
    _assert_same_bits(s1.params, p1, "first held snapshot after the refused take")
    _assert_same_bits(s2.params, p2, "second held snapshot after the refused take")
    s1.release()
    s3 = agent.snapshot(("params",), slots=2)
    _assert_same_bits(s3.params, agent.state.params, "the take after a release")
    _assert_same_bits(s2.params, p2, "the snapshot held across another take")
    assert s1.step < s2.step < s3.step == agent.state.step
    s2.release()
    s3.release()


class _Released:
    """a snapshot as publish_network takes it (wait / params / finite / release), telling the test when it was released"""

    def __init__(self, snap):
        self._snap, self.released = snap, threading.Event()
        self.step = snap.step

    def wait(self):
        return self._snap.wait()

    @property
    def params(self):
        return self._snap.params

    @property
    def finite(self):
        return self._snap.finite

    @property
    def nonfinite(self):
        return self._snap.nonfinite

    def release(self):
        self._snap.release()
        self.released.set()


def _loopback(port):
    from serl_amd.transport import TrainerClient, TrainerServer, make_trainer_config
    cfg = make_trainer_config(port_number=port, broadcast_port=port + 1)
    server = TrainerServer(cfg, transport="loopback")
    server.start(threaded=True)
    client = TrainerClient("actor_env", "localhost", cfg, transport="loopback", wait_for_server=True)
    got = queue.Queue()
    client.recv_network_callback(got.put)
    return server, client, got


def test_nonfinite_values_are_counted_and_keep_the_state_at_home(gpu, tmp_path):
    from serl_amd.utils.checkpoint import save_checkpoint
    agent = _agent("sac")
    core = agent.core
    names = list(core.leaves)
    assert names[-1] == "temp/lagrange"                 # the last leaf of the parameter arena: the scalar tail of its run
    saved = {n: core.get("params", n) for n in ("critic/b1", "temp/lagrange", "critic/w1", "actor/b1")}
    v = saved["critic/b1"].copy(); v[0] = np.nan; core.set("params", "critic/b1", v)                      # first element of a leaf
    v = saved["temp/lagrange"].copy(); v[-1] = np.nan; core.set("params", "temp/lagrange", v)           # last element of the arena
    v = saved["critic/w1"].copy(); v[v.size // 2] = np.inf; v[v.size // 2 + 1] = -np.inf; core.set("params", "critic/w1", v)
    v = saved["actor/b1"].copy(); v[1], v[2], v[3] = 1e-42, -0.0, 3.4e38; core.set("params", "actor/b1", v)   # finite, all three
    snap = agent.snapshot(ALL)
    assert snap.nonfinite == {"params": 4, "target_params": 0, "opt_states": 0} and snap.finite is False
    got = _flat(snap.params)
    assert np.isnan(got[("modules_temperature", "lagrange")]).all() and np.isnan(got[("modules_critic", "network", "Dense_0", "bias")].reshape(-1)[0])
    assert got[("modules_actor", "network", "Dense_0", "bias")].reshape(-1)[1:4].tobytes() == np.array([1e-42, -0.0, 3.4e38], np.float32).tobytes()
    ckpt = tmp_path / "ckpt"
    with pytest.raises(ValueError, match="non-finite"):
        save_checkpoint(str(ckpt), snap, step=snap.step)
    assert not ckpt.exists()
    server, client, inbox = _loopback(6310)
    try:
        handed = _Released(snap)
        server.publish_network(handed)
        assert handed.released.wait(TIMEOUT)
        assert server.stats["publish_refused_nonfinite"] == 1 and server.stats["published"] == 0 and inbox.empty()
        for n, val in saved.items():
            core.set("params", n, val)
        with agent.snapshot(ALL) as clean:
            assert clean.finite and clean.nonfinite == {s: 0 for s in ALL}
            _assert_same_bits(clean.params, agent.state.params, "params after the leaves were restored")
    finally:
        client.stop()
        server.stop()


def test_checkpoint_of_a_snapshot_is_the_agents_file(gpu, tmp_path):
    from serl_amd.utils.checkpoint import restore_checkpoint, save_checkpoint
    agent = _agent("frozen")
    db = _batch(agent)
    for i in range(3):
        _step(agent, db, i)
    step = agent.state.step
    a = save_checkpoint(str(tmp_path / "a"), agent, step=step)
    with agent.snapshot(ALL) as snap:
        assert snap.step == step
        b = save_checkpoint(str(tmp_path / "b"), snap, step=snap.step)
    assert os.path.basename(a) == os.path.basename(b)
    assert open(a, "rb").read() == open(b, "rb").read()
    fresh = _agent("frozen", seed=9)
    restore_checkpoint(b, fresh, restore_rng=True)
    want, got = _state_copy(agent.state), _state_copy(fresh.state)
    assert got["step"] == want["step"] and np.array_equal(got["rng"], want["rng"])
    for name in ALL:
        _assert_same_bits(got[name], want[name], name)


def test_publishing_snapshots_in_a_loop_delivers_the_twins_params(gpu):
    agent, twin = _agent("frozen"), _agent("frozen")
    db = _batch(agent)
    server, client, inbox = _loopback(6320)
    try:
        for i in range(6):
            _step(agent, db, i)
            _step(twin, db, i)
            if i % 2 == 1:
                snap = agent.snapshot()
                handed = _Released(snap)
                server.publish_network(handed)
                snap.wait()
                tree = inbox.get(timeout=TIMEOUT)          # delivered before the next one is handed over: none is dropped
                assert handed.released.wait(TIMEOUT)
                want = twin.state.params
                _assert_same_bits(tree, want, f"network after update {i + 1}")
                # one shared frozen trunk, under the first camera in sorted-key order
                assert "pretrained_encoder" in tree["modules_actor"]["encoder"]["encoder_image"]
        assert server.stats["published"] == 3 and "publish_dropped" not in server.stats and inbox.empty()
    finally:
        client.stop()
        server.stop()


def test_refusals(gpu):
    from serl_amd._lib import SerlError
    agent = _agent("sac")
    for slots in (0, 5):
        with pytest.raises(SerlError, match="slots"):
            agent.snapshot(("params",), slots=slots)
    with pytest.raises(SerlError, match="sections"):
        agent.snapshot(())
    with pytest.raises(KeyError):
        agent.snapshot(("weights",))
    snap = agent.snapshot(("params",))
    with pytest.raises(KeyError, match=r"holds \('params',\)"):
        snap.target_params
    assert np.isfinite(snap.params["modules_temperature"]["lagrange"]).all()
    snap.release()
    snap.release()       # idempotent
    with pytest.raises(RuntimeError, match="released"):
        snap.params
    # include/serl_mi355.h: an agent with a live snapshot handle cannot be destroyed -- SERL_ERR_STATE, the agent stays as it was
    core = agent.core
    assert core.L.serl_agent_destroy(core._h) == -3
    assert b"snapshot" in core.L.serl_last_error()
    with agent.snapshot(("params",)) as again:
        _assert_same_bits(again.params, agent.state.params, "a snapshot after the refused destroy")


@pytest.mark.parametrize("idiom,slots", [("callable", 1), ("callable", 2), ("callable", 3), ("plain", 3)])
def test_a_publisher_that_is_behind_never_fails_the_learner(gpu, monkeypatch, idiom, slots):
    """Three hand-overs of real snapshots while the publisher thread sits in a slow encode of the first.  publish_network(agent.snapshot)
    lets the server take the snapshot after it has released the queued one, and skips a network when every slot is still held: no
    call raises at any number of slots.  publish_network(agent.snapshot()) needs the three slots of the default: one with the
    publisher, one queued, one being taken."""
    from serl_amd.transport import endpoint
    agent = _agent("sac")
    db = _batch(agent)
    server, client, inbox = _loopback(6330 + 2 * slots + (10 if idiom == "plain" else 0))
    entered, go, real, calls = threading.Event(), threading.Event(), endpoint.encode, []

    def slow_encode(msg):
        if isinstance(msg, dict) and "modules_critic" in msg and not calls:      # the first network only
            calls.append(1)
            entered.set()
            assert go.wait(TIMEOUT)
        return real(msg)
    monkeypatch.setattr(endpoint, "encode", slow_encode)
    taken, want = [], []

    def take():
        taken.append(agent.snapshot(("params",), slots=slots))
        return taken[-1]
    try:
        for i in range(3):
            _step(agent, db, i)
            want.append(_copy_tree(agent.state.params))
            server.publish_network(take if idiom == "callable" else agent.snapshot())      # must not raise
            if i == 0:
                assert entered.wait(TIMEOUT)        # the publisher holds the first snapshot from here on
            elif taken and not taken[-1]._released:
                taken[-1].wait()                    # (its copy is complete: a release frees the slot for the next take at once)
        # one slot: both later networks were skipped; more: the second was queued and gave way to the third
        sent = [0] if slots == 1 else [0, 2]
        assert server.stats["publish_dropped"] == 3 - len(sent)
        go.set()
        for i in sent:
            _assert_same_bits(inbox.get(timeout=TIMEOUT), want[i], f"network {i}")
    finally:
        go.set()
        client.stop()
        server.stop()
    assert server.stats["published"] == len(sent) and inbox.empty()
    with agent.snapshot(("params",), slots=slots) as snap:      # every slot came back
        assert snap.finite
