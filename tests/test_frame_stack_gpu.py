"""GPU: frame-stacked observations (num_stack = T > 1) for the SmallEncoder DrQ learner, from the replay store to the update.
EncodingWrapper(enable_stacking=True) folds a stack into the channels and the proprio width (common/encoding.py:39-44,58-64), _unpack
takes observation = frames 0..T-1 and next observation = frames 1..T of the packed window (utils/train_utils.py:53-64), and the
random shift gives frame (b, t) the offset of key b*T + t (vision/data_augmentations.py:22-36, num_batch_dims=2).  References: the
NumPy replay oracle (bytes: exact), oracle/drq_oracle.py widened by tests/stacked_oracle.py (fp64; tolerances imported from
tests/test_small_encoder_gpu.py), and tests/golden/stack2_update_drq_small.npz, a run of the reference's own DrQAgent at T = 2."""
import itertools

import numpy as np
import pytest
import torch

from helpers import make_spaces
from oracle import drq_oracle as O
from oracle import ref_update_runner as RR
from oracle.replay_oracle import ReplayOracle
import agent_helpers as AH
import stacked_oracle as SO
from test_small_encoder_gpu import ALL_NETS, TOL, _compare_state

pytestmark = pytest.mark.gpu
KEYS = ("front", "wrist")


def _leaves(core):
    out = {}
    for sec in ["params", "target_params"] + [f"opt/{tx}/{m}" for tx in ("actor", "critic", "temperature") for m in ("mu", "nu")]:
        for leaf in core.leaves:
            if sec.startswith("opt/") and leaf.startswith("trunk/"):      # the frozen trunk has no moments
                continue
            out[(sec, leaf)] = core.get(sec, leaf).copy()
    return out


def _same_bits(a, b):
    assert a.keys() == b.keys()
    bad = [k for k in a if not np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32))]
    assert not bad, bad[:5]


def _sample_obs(T, H, W, S):
    obs = {k: np.zeros((T, H, W, 3), np.uint8) for k in KEYS}
    obs["state"] = np.zeros((T, S), np.float32)
    return obs


def _stacked_agent(T, B, seed=0, H=64, W=64, S=5, A=3, **kw):
    from serl_amd.utils.launcher import make_drq_agent
    return make_drq_agent(seed, _sample_obs(T, H, W, S), np.zeros((A,), np.float32), image_keys=KEYS, encoder_type="small", batch_size=B, **kw)


# ------------------------------------------------------------------------------------------------------------------ 1. gather + crop
def _filled(T, H, W, ep, seed, n=85, cap=64, S=5, A=3):
    """a store and its oracle after `n` inserts: past one wrap of the 64-slot ring (every insert of an episode's first
    transition also writes T first-frame slots)"""
    from serl_amd.data.data_store import MemoryEfficientReplayBufferDataStore
    from serl_amd.utils.synthetic import transition_stream
    osp, asp = make_spaces(KEYS, H, W, 3, T, S, A)
    rb = MemoryEfficientReplayBufferDataStore(osp, asp, cap, image_keys=KEYS)
    o = ReplayOracle(KEYS, H, W, 3, T, S, A, cap)
    for tr in itertools.islice(transition_stream(KEYS, H, W, 3, T, S, A, ep, seed), n):
        rb.insert(tr)
        o.insert(tr)
    assert len(rb) == cap and (rb.valid_mask() == o.valid).all()
    return rb, o


def _three(o, T):
    """three valid slots: the lowest (below T where the ring has one: numpy's negative-window wrap), one right behind an
    invalid slot (first-frame slots or the wrap's copies inside its window), the highest"""
    v = np.flatnonzero(o.valid)
    behind = [i for i in v if i >= T and not o.valid[i - 1]]
    return np.array([v[0], behind[0], v[-1]], np.int64)


@pytest.mark.parametrize("T,H,W,ep_b", [(2, 40, 32, 7), (3, 33, 48, 6)])
def test_gather_crop_of_stacks_is_byte_exact(gpu, T, H, W, ep_b):
    """Two stores (RLPD split 3 + 3), capacity 64, filled past one wrap with episodes of 7 (the second store of the T = 3 case
    with episodes of 6: with 7 no valid slot below T ever arises in a 64-slot ring at T = 3, with 6 slot 0 is one), against
    ReplayOracle.gather + _unpack + the per-frame edge-replicated shift; then the same crop through serl_crop_packed_stacked on
    the packed gather's output."""
    import ctypes as C
    from serl_amd import _lib
    from serl_amd.agents.batch import DeviceBatch
    from serl_amd.data.data_store import gather_crop
    S, A, B = 5, 3, 6
    (ra, oa), (rb, ob) = _filled(T, H, W, 7, 11), _filled(T, H, W, ep_b, 12)
    ia, ib = _three(oa, T), _three(ob, T)
    assert min(ia.min(), ib.min()) < T, "no sampled slot below T: the negative-window wrap is not exercised"
    rng = np.random.default_rng(5)
    co, cn = rng.integers(0, 9, (B * T, 2)).astype(np.int32), rng.integers(0, 9, (B * T, 2)).astype(np.int32)
    corners = [(0, 0), (8, 8), (0, 8), (8, 0)]
    for t in range(T):      # the frames of one sample take different corners: key b*T + t, not b
        co[0 * T + t], co[2 * T + t], cn[4 * T + t] = corners[t], corners[(t + 2) % 4], corners[(t + 1) % 4]
    packed = {k: np.concatenate([oa.gather(ia)["observations"][k], ob.gather(ib)["observations"][k]]) for k in KEYS}
    want = {"obs": {k: SO.shift_stack(packed[k][:, :T], co) for k in KEYS}, "next": {k: SO.shift_stack(packed[k][:, 1:], cn) for k in KEYS}}
    per_sample = SO.shift_stack(packed["front"][:, :T], np.repeat(co[::T], T, 0))       # what key b (one offset per stack) would give
    assert (per_sample[0, 0] == want["obs"]["front"][0, 0]).all() and not (per_sample[0, 1] == want["obs"]["front"][0, 1]).all()
    out = DeviceBatch(B, 2, H, W, 3, T * S, A, 0, num_stack=T)
    ia_in, ib_in = ia.copy(), ib.copy()
    gather_crop([(ra, ia_in), (rb, ib_in)], co, cn, out)
    torch.cuda.synchronize()
    assert (ia_in == ia).all() and (ib_in == ib).all()          # nothing was stale: the in/out indices came back as given
    fr = out.frames.cpu().numpy()
    assert fr.shape == (2, 2, B, T, H, W, 3)
    for c, k in enumerate(KEYS):
        assert (fr[0, c] == want["obs"][k]).all() and (fr[1, c] == want["next"][k]).all(), k
    ga, gb = oa.gather(ia), ob.gather(ib)
    cat = lambda f: np.concatenate([f(ga), f(gb)])      # noqa: E731
    assert (out.state[0].cpu().numpy() == cat(lambda g: g["observations"]["state"]).reshape(B, -1)).all()
    assert (out.state[1].cpu().numpy() == cat(lambda g: g["next_observations"]["state"]).reshape(B, -1)).all()
    assert (out.action.cpu().numpy() == cat(lambda g: g["actions"])).all()
    assert (out.reward.cpu().numpy() == cat(lambda g: g["rewards"])).all()
    assert (out.mask.cpu().numpy() == cat(lambda g: g["masks"])).all()
    assert (out.done.cpu().numpy().astype(bool) == cat(lambda g: g["dones"])).all()
    # the packed gather's output through the stand-alone crop
    pa, pb = ra.gather(ia), rb.gather(ib)
    dev_packed = [torch.cat([pa["observations"][k], pb["observations"][k]]).contiguous() for k in KEYS]
    assert all((p.cpu().numpy() == packed[k]).all() for p, k in zip(dev_packed, KEYS))
    out2 = torch.zeros_like(out.frames)
    ptrs = (C.c_void_p * 2)(*[p.data_ptr() for p in dev_packed])
    s = torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.lib().serl_crop_packed_stacked(0, ptrs, 2, B, T, H, W, 3, co.ctypes.data, cn.ctypes.data, out2.data_ptr(), C.c_void_p(s)))
    torch.cuda.synchronize()
    assert torch.equal(out2, out.frames)
    # no table = the identity shift: _unpack alone
    _lib.check(_lib.lib().serl_crop_packed_stacked(0, ptrs, 2, B, T, H, W, 3, None, None, out2.data_ptr(), C.c_void_p(s)))
    torch.cuda.synchronize()
    for c, k in enumerate(KEYS):
        assert (out2[0, c].cpu().numpy() == packed[k][:, :T]).all() and (out2[1, c].cpu().numpy() == packed[k][:, 1:]).all()


# ------------------------------------------------------------------------------------------------------------------ 2. layer 0
@pytest.mark.parametrize("H,W", [(33, 47), (64, 64)])
@pytest.mark.parametrize("T", [2, 3, 4])
def test_layer0_forward_and_weight_gradient(gpu, T, H, W):
    """SmallEncoder layer 0 on 3T channels read from the planar frames: its ReLU output (tap small_act0) and the gradient of its
    kernel and bias in one critic step, against fp64.  One frame of every stack is all 255 and another all 0, so an output
    computed with t and the tap swapped, or a gradient row filed under another frame, cannot pass."""
    B = 3
    cfg = SO.config(KEYS, H, W, 4, 3, T)
    st, core = SO.make_pair(cfg, T, B)
    pb = SO.synth_packed_batch(cfg, T, B, seed=20 + T)
    for k in KEYS:      # observation frames 0 and 1 of every stack (next frame 0 is packed frame 1)
        pb["frames"][k][:, 0], pb["frames"][k][:, 1] = 0, 255
    noise = SO.make_noise(cfg, T, B, seed=9)
    fr = SO.cropped(cfg, T, pb, noise["crop_obs"], noise["crop_next"])
    b, tn = SO.oracle_batch(cfg, T, pb, fr), O.noise_to_torch(noise, torch.float64)
    act0 = {k: torch.relu(O.conv_nhwc(b["obs"][k].to(torch.float64) / 255.0, st.params[f"enc/{k}/conv0/kernel"], 2, ((0, 0), (0, 0)))
                          + st.params[f"enc/{k}/conv0/bias"]).numpy() for k in KEYS}
    info, aux = O.update_critics(st, b, tn)
    core.update_critics(SO.device_batch(cfg, T, pb, fr), AH.noise_to_device(cfg, noise))
    h1, w1 = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    got = core.debug("small_act0", 2 * B * h1 * w1 * 32).reshape(2, B, h1, w1, 32)      # the last pass: online encoder at obs
    for c, k in enumerate(KEYS):
        e = AH.rel_err(got[c], act0[k])
        print(f"layer 0 forward T={T} {H}x{W} {k}: {e:.2e}")
        assert e < TOL, (k, e)
    g0 = {k: v for k, v in aux["grads"].items() if "/conv0/" in k}
    assert len(g0) == 4 and g0["enc/front/conv0/kernel"].shape == (3, 3, 3 * T, 32)
    worst = SO.check_grads(cfg, T, core, g0, "g_critic", 0, TOL)
    print(f"layer 0 weight gradient T={T} {H}x{W}: {worst:.2e}")
    got_info = core.read_info()
    for k in ("critic_loss", "predicted_qs", "target_qs"):
        assert abs(got_info[k] - info[k]) < TOL * max(1.0, abs(info[k])), (k, got_info[k], info[k])


# ------------------------------------------------------------------------------------------------------------------ 3. update parity
def test_updates_match_the_fp64_restatement_at_num_stack_2(gpu):
    """update_critics, update_high_utd(utd_ratio=2) and update at T = 2, B = 6, 64x64 with injected noise: infos, Q values, the
    encoder output, every gradient leaf and the parameters, at the figures of tests/test_small_encoder_gpu.py"""
    T, B = 2, 6
    cfg = SO.config(KEYS, 64, 64, 5, 3, T)
    st, core = SO.make_pair(cfg, T, B)
    sl, _ = SO.leaf_slices(cfg, T)
    for it, kind in enumerate(("critics", "high_utd", "update", "critics")):
        utd = 2 if kind == "high_utd" else 1
        pb = SO.synth_packed_batch(cfg, T, B, seed=40 + it)
        noise = SO.make_noise(cfg, T, B, seed=50 + it, utd_ratio=utd)
        fr = SO.cropped(cfg, T, pb, noise["crop_obs"], noise["crop_next"])
        tb, tn = SO.oracle_batch(cfg, T, pb, fr), O.noise_to_torch(noise, torch.float64)
        db, dn = SO.device_batch(cfg, T, pb, fr), AH.noise_to_device(cfg, noise)
        info, aux = RR.run_step(st, {"kind": kind, "utd": utd, "nets": ALL_NETS}, tb, tn)
        if kind == "critics":
            core.update_critics(db, dn)
            if it == 0:
                q = core.debug("q", cfg.ensemble * B).reshape(cfg.ensemble, B)
                assert AH.rel_err(q, aux["q"].numpy()) < TOL
                assert AH.rel_err(core.debug("target_q", B), aux["target_q"].numpy()) < TOL
                x = core.debug("x", B * (cfg.enc_dim + cfg.A)).reshape(B, -1)
                assert AH.rel_err(x[:, :cfg.enc_dim], aux["enc_obs"].numpy()) < TOL
                assert "enc/front/conv0/kernel" in aux["grads"] and "enc/proprio/dense/kernel" in aux["grads"]
                SO.check_grads(cfg, T, core, aux["grads"], "g_critic", 0, TOL)
        elif kind == "high_utd":
            core.update_high_utd(db, utd, dn)
            SO.check_grads(cfg, T, core, aux["g_actor"], "g_actor", sl["enc/proprio/dense/kernel"][0], TOL)
        else:
            core.update(db, ALL_NETS, dn)
        got = core.read_info()
        for k, v in info.items():
            assert abs(got[k] - v) < 2 * TOL * max(1.0, abs(v)), (it, kind, k, got[k], v)
    _compare_state(cfg, st, core, steps=6)
    assert core.step == st.step == 6    # 1 + (2 + 1) + 1 + 1 optimizer steps


@pytest.mark.parametrize("noise_form", ["keys", "tensors"])
def test_agent_reproduces_the_reference_golden_from_the_seed(gpu, noise_form):
    """tests/golden/stack2_update_drq_small.npz: nothing injected -- the B*T crop offsets per stream, the REDQ indices and the
    normals are drawn in the library from state.rng.  Tolerances: those tests/test_golden_update_gpu.py applies to a seed-only
    SmallEncoder golden."""
    from oracle import golden_update as G
    g = SO.unpack(np.load(SO.golden_path()))
    cfg, T, B = g["cfg"], g["T"], g["B"]
    agent = _stacked_agent(T, B, seed=0, S=cfg.S // T, discount=cfg.discount)
    SO.load_theta(agent.core, cfg, SO.init_params(cfg, T, g["meta"]["param_seed"]))
    agent.noise_form = noise_form
    assert agent.rng_impl == "threefry" and agent.num_stack == T
    assert [int(v) for v in agent.state.rng] == g["meta"]["rng0"]
    n_steps = 0
    for i, step in enumerate(g["steps"]):
        batch = SO.reference_batch(cfg, T, step["batch"], unpacked=step["kind"] == "update")
        if step["kind"] == "critics":
            agent, info = agent.update_critics(batch)
            flat = dict(info["critic"])
            n_steps += 1
        elif step["kind"] == "high_utd":
            agent, info = agent.update_high_utd(batch, utd_ratio=step["utd"])
            flat = {**info["critic"], **info["actor"], **info["temperature"]}
            n_steps += step["utd"] + 1
        else:
            agent, info = agent.update(batch, networks_to_update=frozenset(step["nets"]))
            flat = {**info["critic"], **info["actor"], **info["temperature"]}
            n_steps += 1
        d, want = agent.last_draws, step["noise"]
        if "crop_obs" in want:
            assert d["crop_obs"].shape == (B * T, 2)
            assert np.array_equal(d["crop_obs"], want["crop_obs"]) and np.array_equal(d["crop_next"], want["crop_next"]), "crop offsets"
        assert np.array_equal(d["redq_idx"], np.asarray(want["redq_idx"], np.int32).reshape(d["redq_idx"].shape)), "REDQ indices"
        for tx in ("actor", "critic", "temperature"):
            flat[f"{tx}_lr"] = info[f"{tx}_lr"]
        for k, r in step["info"].items():
            assert abs(flat[k] - r) < TOL * max(1.0, abs(r)), (i, step["kind"], k, flat[k], r)
    assert agent.state.step == g["meta"]["final_step"] == n_steps
    assert [int(v) for v in agent.state.rng] == g["meta"]["rng_final"], "state.rng did not advance as the reference's"
    assert G.shape_tree(agent.state.params) == g["meta"]["param_tree"]
    assert G.shape_tree(agent.state.target_params) == g["meta"]["param_tree"]
    assert G.shape_tree(agent.state.opt_states) == g["meta"]["opt_state_tree"]
    core, worst_m, worst_p = agent.core, 0.0, 0.0
    for name in SO.param_shapes(cfg, T):
        leaf = SO.product_name(name, cfg.image_keys)
        for tx in ("critic", "actor", "temperature"):
            for mom in ("mu", "nu"):
                err, scale = SO.leaf_errors(f"{mom}_{tx}/{name}", g["final"][f"{mom}_{tx}"][name], core.get(f"opt/{tx}/{mom}", leaf))
                if scale < 1e-200:       # outside this optimizer's support: exactly zero on both sides
                    assert err.max() == 0.0, (tx, mom, name)
                    continue
                worst_m = max(worst_m, err.max() / scale)
                assert err.max() / scale < 3 * TOL, (tx, mom, name, err.max() / scale)      # a seed-only run's bound there
        for sec, gsec in (("params", "params"), ("target_params", "target")):
            err, scale = SO.leaf_errors(f"{gsec}/{name}", g["final"][gsec][name], core.get(sec, leaf))
            bulk = float(np.quantile(err, 0.999)) / scale
            worst_p = max(worst_p, bulk)
            assert bulk < TOL, (sec, name, bulk)
            bound = 2.1 * cfg.lr * n_steps * (cfg.tau * n_steps if sec == "target_params" else 1.0) + TOL * scale
            assert err.max() <= bound, (sec, name, err.max(), bound)
    print(f"stack2 golden ({noise_form}): Adam moments {worst_m:.1e}, params (99.9 pct) {worst_p:.1e}")


# ------------------------------------------------------------------------------------------------------------------ 4. store -> update
def test_store_to_update_equals_the_packed_dict(gpu):
    from serl_amd.data.data_store import LazyBatch, MemoryEfficientReplayBufferDataStore
    from serl_amd.utils.synthetic import transition_stream
    T, B, H, W, S, A = 2, 6, 64, 64, 5, 3
    osp, asp = make_spaces(KEYS, H, W, 3, T, S, A)
    rb = MemoryEfficientReplayBufferDataStore(osp, asp, 100, image_keys=KEYS)
    rb.seed(0)
    for tr in itertools.islice(transition_stream(KEYS, H, W, 3, T, S, A, 9, 5), 70):
        rb.insert(tr)
    a1, a2 = _stacked_agent(T, B, seed=3), _stacked_agent(T, B, seed=3)
    _same_bits(_leaves(a1.core), _leaves(a2.core))
    lazy = rb.sample(B, lazy=True)
    assert isinstance(lazy, LazyBatch)
    idx = lazy.parts[0][1].copy()
    packed = rb.gather(idx)
    assert packed["observations"]["front"].shape == (B, T + 1, H, W, 3) and packed["observations"]["state"].shape == (B, T, S)
    keep = {k: v.clone() for k, v in packed["observations"].items()}
    count, mask = rb.insert_count(), rb.valid_mask()
    a1, i1 = a1.update_critics(lazy)
    a2, i2 = a2.update_critics(packed)
    assert a1.last_draws["crop_obs"].shape == (B * T, 2) and np.array_equal(a1.last_draws["crop_obs"], a2.last_draws["crop_obs"])
    assert dict(i1["critic"]) == dict(i2["critic"]) and np.isfinite(i1["critic"]["critic_loss"])
    _same_bits(_leaves(a1.core), _leaves(a2.core))
    assert np.array_equal(a1.state.rng, a2.state.rng) and a1.state.step == 1
    # neither the caller's batch nor the store was written
    assert (lazy.parts[0][1] == idx).all() and all(torch.equal(packed["observations"][k], v) for k, v in keep.items())
    again = rb.gather(idx)
    assert all(torch.equal(again["observations"][k], v) for k, v in keep.items())
    assert rb.insert_count() == count and (rb.valid_mask() == mask).all()
    # the unpacked form of the same sample is the same batch; two views that are not one window are refused
    a3 = _stacked_agent(T, B, seed=3)
    obs = {k: (v if k == "state" else v[:, :T]) for k, v in packed["observations"].items()}
    nobs = {k: packed["observations"][k][:, 1:] for k in KEYS}
    nobs["state"] = packed["next_observations"]["state"]
    unpacked = dict(packed, observations=obs, next_observations=nobs)
    a3, _ = a3.update_critics(unpacked)
    _same_bits(_leaves(a1.core), _leaves(a3.core))
    bad = dict(unpacked, next_observations=dict(nobs, front=nobs["front"].flip(1)))
    with pytest.raises(ValueError, match="packed window"):
        a3.update_critics(bad)
    assert a3.state.step == 1


# ------------------------------------------------------------------------------------------------------------------ 5. acting
def test_sample_actions_at_num_stack_2(gpu):
    from serl_amd import jaxrng as J
    T, H, W, S, A = 2, 64, 64, 5, 3
    cfg = SO.config(KEYS, H, W, S, A, T)
    agent = _stacked_agent(T, 8, seed=1)
    theta = SO.init_params(cfg, T, 7)
    SO.load_theta(agent.core, cfg, theta)
    th = O.to_torch(theta, torch.float64)
    rng = np.random.default_rng(2)
    n = 4
    obs = {k: rng.integers(0, 256, (n, T, H, W, 3), dtype=np.uint8) for k in KEYS}
    obs["state"] = rng.standard_normal((n, T, S)).astype(np.float32)
    enc = O.encode(th, cfg, {k: torch.from_numpy(SO.fold(obs[k])) for k in KEYS}, torch.tensor(obs["state"].reshape(n, -1), dtype=torch.float64))
    mean, std = O.policy_head(th, cfg, enc)
    mode = agent.sample_actions(obs, argmax=True)
    assert mode.shape == (n, A) and AH.rel_err(mode, torch.tanh(mean).numpy()) < TOL
    one = {k: v[2] for k, v in obs.items()}                 # a single observation: (T, H, W, 3) frames, a (T, S) state
    m1 = agent.sample_actions(one, argmax=True)
    assert m1.shape == (A,) and AH.rel_err(m1, torch.tanh(mean[2]).numpy()) < TOL
    key = J.prngkey(5)
    eps = J.normal_host(key, n * A).reshape(n, A)
    want, _ = O.sample_and_log_prob(mean, std, torch.tensor(eps, dtype=torch.float64))
    got = agent.sample_actions(obs, seed=key)
    assert AH.rel_err(got, want.numpy()) < TOL
    w1, _ = O.sample_and_log_prob(mean[2:3], std[2:3], torch.tensor(J.normal_host(key, A).reshape(1, A), dtype=torch.float64))
    assert AH.rel_err(agent.sample_actions(one, seed=key), w1.numpy()[0]) < TOL


# ------------------------------------------------------------------------------------------------------------------ 6. T = 1 unchanged
@pytest.mark.parametrize("encoder_type", ["small", "resnet-pretrained"])
def test_num_stack_1_given_explicitly_is_the_agent_it_was(gpu, encoder_type):
    """num_stack = 1 and num_stack = 0 (a zero-initialised field) are the same agent: parameters, infos, state.rng and the
    number of update-chain launches, bit for bit, over update_critics + update_high_utd from the seed"""
    from serl_amd import _lib
    from serl_amd.agents.core import AgentCore
    from serl_amd.agents.drq import DrQAgent
    B = 8
    cfg = O.Config(image_keys=KEYS, H=64, W=64, S=5, A=3, encoder_type=encoder_type)
    trunk, theta = O.init_params(cfg, 42)
    pbs = [SO.synth_packed_batch(cfg, 1, B, seed=70 + i) for i in range(2)]
    runs = []
    for num_stack in (0, 1):
        core = AgentCore(encoder_type=encoder_type, n_cam=2, H=64, W=64, state_dim=5, act_dim=3, batch=B, seed=0, num_stack=num_stack)
        assert core.leaves["enc/0/conv0/kernel" if encoder_type == "small" else "enc/0/dense/kernel"] > 0
        for sec in ("params", "target_params"):
            core.load_flat(sec, trunk)
            core.load_flat(sec, {AH.product_name(k, KEYS): v for k, v in theta.items()})
        agent = DrQAgent(core, KEYS, {}, 0)
        assert agent.num_stack == 1
        n0 = int(_lib.lib().serl_debug_chain_launches())
        agent, ic = agent.update_critics(SO.reference_batch(cfg, 1, pbs[0]))
        ic = dict(ic["critic"])
        agent, ih = agent.update_high_utd(SO.reference_batch(cfg, 1, pbs[1]), utd_ratio=2)
        ih = {**ih["critic"], **ih["actor"], **ih["temperature"]}
        torch.cuda.synchronize()
        runs.append((_leaves(core), ic, ih, agent.state.rng.copy(), int(_lib.lib().serl_debug_chain_launches()) - n0, core.step))
    (l0, c0, h0, r0, n0, s0), (l1, c1, h1, r1, n1, s1) = runs
    _same_bits(l0, l1)
    assert c0 == c1 and h0 == h1 and np.array_equal(r0, r1) and n0 == n1 > 0 and s0 == s1 == 4
    if encoder_type == "small":
        assert l1[("params", "enc/0/conv0/kernel")].size == 27 * 32


# ------------------------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_name_their_reason_and_step_nothing(gpu):
    from serl_amd._lib import SerlError
    from serl_amd.agents.batch import DeviceBatch
    from serl_amd.agents.core import AgentCore
    from serl_amd.data.data_store import MemoryEfficientReplayBufferDataStore, gather_crop
    from serl_amd.networks.reward_classifier import Classifier
    from serl_amd.utils.launcher import make_drq_agent
    T, B, H, W, S, A = 2, 4, 64, 64, 5, 3
    with pytest.raises(SerlError, match=r"conv_init kernel is \(7,7,3,64\)"):        # the frozen trunk cannot take a stack
        AgentCore(encoder_type="resnet-pretrained", n_cam=2, H=H, W=W, state_dim=T * S, act_dim=A, batch=B, num_stack=T)
    with pytest.raises(NotImplementedError, match="conv_init"):
        make_drq_agent(0, _sample_obs(T, H, W, S), np.zeros((A,), np.float32), image_keys=KEYS, encoder_type="resnet-pretrained", batch_size=B)
    with pytest.raises(SerlError, match=r"num_stack 5 not in \[1,4\]"):
        AgentCore(encoder_type="small", n_cam=2, H=H, W=W, state_dim=5 * S, act_dim=A, batch=B, num_stack=5)
    agent = _stacked_agent(T, B, seed=2)
    core = agent.core
    before = _leaves(core)
    # a batch of single frames (same state width) handed to the stacked agent
    db = DeviceBatch(B, 2, H, W, 3, T * S, A, 0, num_stack=1)
    for t in (db.frames, db.state, db.action, db.reward, db.mask, db.done):
        t.zero_()
    for call in (lambda: core.update_critics(db), lambda: core.update_high_utd(db, 2), lambda: core.update(db)):
        with pytest.raises(SerlError, match="num_stack 1 does not match the agent's num_stack 2"):
            call()
    # a store of stacks of 2 gathered into a single-frame batch, and a stack-of-2 batch from a single-frame store
    osp, asp = make_spaces(KEYS, H, W, 3, T, S, A)
    rb = MemoryEfficientReplayBufferDataStore(osp, asp, 50, image_keys=KEYS)
    rb.seed(0)
    from serl_amd.utils.synthetic import transition_stream
    for tr in itertools.islice(transition_stream(KEYS, H, W, 3, T, S, A, 9, 5), 20):
        rb.insert(tr)
    idx = rb.sample_indices(B)
    with pytest.raises(SerlError, match="the store holds stacks of 2 frames, serl_batch.num_stack is 1"):
        gather_crop([(rb, idx)], None, None, db)
    osp1, asp1 = make_spaces(KEYS, H, W, 3, 1, T * S, A)
    rb1 = MemoryEfficientReplayBufferDataStore(osp1, asp1, 50, image_keys=KEYS)
    rb1.seed(0)
    for tr in itertools.islice(transition_stream(KEYS, H, W, 3, 1, T * S, A, 9, 5), 20):
        rb1.insert(tr)
    db2 = DeviceBatch(B, 2, H, W, 3, T * S, A, 0, num_stack=T)
    with pytest.raises(SerlError, match="the store holds stacks of 1 frames, serl_batch.num_stack is 2"):
        gather_crop([(rb1, rb1.sample_indices(B))], None, None, db2)
    # the reward classifier reads single frames
    with pytest.raises(SerlError, match="reads single frames"):
        agent.set_reward_classifier(Classifier(KEYS, H, W, max_batch=B))
    assert agent.reward_classifier is None and core.step == 0
    _same_bits(before, _leaves(core))


# ------------------------------------------------------------------------------------------------------------------ 8. checkpoint
def test_checkpoint_of_a_stacked_agent_continues_bit_identically(gpu, tmp_path):
    from serl_amd.utils.checkpoint import restore_checkpoint, save_checkpoint
    T, B, K = 2, 6, 2
    cfg = SO.config(KEYS, 64, 64, 5, 3, T)
    batches = [SO.synth_packed_batch(cfg, T, B, seed=90 + i) for i in range(2 * K)]

    def step(agent, i):
        batch = SO.reference_batch(cfg, T, batches[i])
        return (agent.update_critics(batch) if i % 2 == 0 else agent.update_high_utd(batch, utd_ratio=2))[0]

    whole = _stacked_agent(T, B, seed=4)
    for i in range(2 * K):
        whole = step(whole, i)
    first = _stacked_agent(T, B, seed=4)
    for i in range(K):
        first = step(first, i)
    save_checkpoint(str(tmp_path), first, step=int(first.state.step))
    resumed = restore_checkpoint(str(tmp_path), _stacked_agent(T, B, seed=77), restore_rng=True)
    assert resumed.state.params["modules_actor"]["encoder"]["encoder_front"]["Conv_0"]["kernel"].shape == (3, 3, 3 * T, 32)
    assert resumed.state.params["modules_actor"]["encoder"]["Dense_0"]["kernel"].shape == (T * 5, 64)
    for i in range(K, 2 * K):
        resumed = step(resumed, i)
    _same_bits(_leaves(whole.core), _leaves(resumed.core))
    assert np.array_equal(whole.state.rng, resumed.state.rng) and whole.state.step == resumed.state.step == 8
