"""GPU: Dropout in the critic's and the policy's MLP (serl_agent_create_dropout; the `drop` field of LnFwdArgs / LnBwdArgs in
serl_amd/csrc/heads.hip: ln_dropout in ln_row and ln_bwd_row; serl_mlp_noise) -- tests/mlp_dropout.py.

* the reference's own update code with a dropout_rate (tests/golden/drop_*.npz, every recorded draw injected) through
  tests/golden_replay.py::replay in both schedules: its comparisons, its TOL;
* the same files from the seed alone, the masks drawn from the call's keys in the LayerNorm rows ("keys") or filled as tensors
  ("tensors"): the two forms leave the same bytes;
* one layer at each row layout (width 64, blocked 256, strided 192) on 6 and 37 rows per minibatch of an update_high_utd(2), one
  group (policy) and three (critic): where the mask is 0 the gradient wrt the Dense output and a fully dropped column's bias and
  kernel gradients are exactly 0, everything else matches the fp64 statement;
* evaluate_losses reports the update's info; q_values, policy_stats and sample_actions ignore the rates and write nothing;
* a rate-0 agent through serl_agent_create_dropout is serl_agent_create_mlp's, bit for bit;
* two shards of a batch through the phase API sum to the full batch, under "keys" and under the device hash;
* the hash stream: kept fractions, forward and backward agreeing on every element, members sharing the mask."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import drq_oracle as O
import agent_helpers as AH
import golden_replay as GR
import mlp_dropout as MD
from serl_amd import jaxrng as J
from test_agent_gpu import TOL, _compare_state
from test_mlp_widths_gpu import _Figures, _grads, _info

pytestmark = pytest.mark.gpu
NAMES = list(MD.GOLDEN)
SECTIONS = ("params", "target_params", "opt/critic/mu", "opt/critic/nu", "opt/actor/mu", "opt/actor/nu", "opt/temperature/mu", "opt/temperature/nu")


def _bits(core):
    return {(sec, leaf): core.get(sec, leaf).copy() for leaf in core.leaves for sec in SECTIONS}


def _same_bits(got, want, what=""):
    for key, v in got.items():
        assert np.array_equal(v.view(np.uint32), want[key].view(np.uint32)), (what, key)


def _fixture_agent(name, fuse=None):
    g, meta, _ = GR.load_variant("drop", name)
    cfg, rates = g["cfg"], MD.GOLDEN[name]["rates"]
    with AH.chain_fuse(fuse):
        agent = GR.reference_agent(cfg, g["B"], critic_ensemble_size=cfg.ensemble,
                                   critic_network_kwargs=MD.network_kwargs(cfg, "critic", rates[0]),
                                   policy_network_kwargs=MD.network_kwargs(cfg, "policy", rates[1]), mlp_dropout=True)
    assert (agent.config["critic_dropout_rate"], agent.config["policy_dropout_rate"]) == rates
    assert (agent.core.critic_dropout, agent.core.policy_dropout) == rates and agent.core.cfg.ensemble == cfg.ensemble
    AH.load_leaves(agent.core, cfg, *GR.initial_leaves(cfg, lambda th, c: {k: np.array(v, np.float32) for k, v in th.items()}))
    return agent, g, meta


def _core(cfg, B, rates, fuse=None, agent_seed=0):
    """AH.make_core with the two Dropout rates"""
    from serl_amd.agents.core import AgentCore
    with AH.chain_fuse(fuse):
        return AgentCore(encoder_type=cfg.encoder_type, n_cam=cfg.n_cam, H=cfg.H, W=cfg.W, state_dim=cfg.S, act_dim=cfg.A, batch=B,
                         ensemble=cfg.ensemble, hidden=cfg.hidden, discount=cfg.discount, tau=cfg.tau, lr=cfg.lr, warmup_steps=cfg.warmup,
                         dropout=cfg.dropout, std_min=cfg.std_min, std_max=cfg.std_max, target_entropy=cfg.target_entropy, seed=agent_seed,
                         temp_warmup_steps=-1 if cfg.temp_warmup is None else cfg.temp_warmup, critic_subsample_size=cfg.subsample,
                         backup_entropy=cfg.backup_entropy, optimizers=cfg.opt, critic_activation=cfg.critic_activation,
                         policy_activation=cfg.policy_activation, critic_dropout=rates[0], policy_dropout=rates[1])


# ---- the reference's own code with a dropout_rate ----------------------------------------------------------------------------------
def test_create_states_accepts_a_dropout_rate(gpu):
    """with the switch on; without it the refusal is the one it was (tests/test_mlp_dropout_cpu.py)"""
    from serl_amd.agents.sac import SACAgent
    agent = SACAgent.create_states(0, np.zeros((10,), np.float32), np.zeros((4,), np.float32), critic_network_kwargs={"dropout_rate": 0.1},
                                   batch_size=8, mlp_dropout=True)
    assert agent.config["critic_dropout_rate"] == 0.1 and agent.config["policy_dropout_rate"] == 0.0
    assert abs(agent.core.critic_dropout - 0.1) < 1e-12


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "one_per_operation"])
@pytest.mark.parametrize("name", NAMES)
def test_hip_update_matches_the_reference_golden_with_dropout(gpu, name, fuse):
    agent, g, _ = _fixture_agent(name, fuse)
    GR.replay(MD.Injecting(agent, g["steps"], g["cfg"].hidden), g, label=f"drop_{name}")
    assert agent.core.debug("ctr_nonzero", 1)[0] == 0


def test_replay_without_the_masks_misses_the_golden(gpu):
    """the comparison can tell: the same agent with its masks left to the device hash is far from the recorded run"""
    agent, g, _ = _fixture_agent(NAMES[0])
    with pytest.raises(AssertionError):
        GR.replay(agent, g, label="drop_without_masks")


@pytest.mark.parametrize("name", NAMES)
def test_from_the_seed_both_noise_forms_reproduce_the_golden_bit_equal(gpu, name):
    """Nothing injected: the agent draws crop offsets, REDQ indices, normals, camera masks and MLP masks from state.rng.  The
    policy's Dropout keys come from the library's own scope path; the critic's from the stand-in's, passed in as data (the
    recording's vmapped critic binds its members at a fresh root -- DESIGN.md section 7)."""
    ends = {}
    for form in ("keys", "tensors"):
        agent, g, meta = _fixture_agent(name)
        cfg = g["cfg"]
        agent.noise_form = form
        agent._rng_key = np.array(meta["rng0"], np.uint32)
        agent._call_noise.mlp_dropout_path = lambda net, l: (J.mlp_dropout_path(net, l) if net == "policy" else
                                                             MD.standin_dropout_path(net, l, cfg.state_only))
        GR.replay(agent, g, seed_only=True, label=f"drop_{name} from the seed, {form}")
        if form == "tensors":      # the filled tensors are the recorded masks, bit for bit
            last = g["steps"][-1]
            for site, m in MD.unpack(last["noise"], g["B"], cfg.hidden).items():
                assert np.array_equal(agent._noise_bufs[g["B"]]["drop_mask_" + site].cpu().numpy(), m), site
        ends[form] = _bits(agent.core)
    _same_bits(ends["keys"], ends["tensors"], "keys vs tensors")


# ---- one layer at each row layout --------------------------------------------------------------------------------------------------
LAYERS = [(64, 6), (64, 37), (256, 6), (256, 37), (192, 6), (192, 37)]


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "one_per_operation"])
@pytest.mark.parametrize("D,mb", LAYERS, ids=[f"w{d}_mb{m}" for d, m in LAYERS])
def test_rows_apply_the_mask_forward_and_backward(gpu, D, mb, fuse):
    """update_high_utd(2): the second minibatch's rows start at row mb of every mask.  Column DEAD is dropped in every row of every
    mask: its Dense bias and kernel column receive exactly 0."""
    cfg = O.Config(image_keys=(), S=10, A=3, discount=0.99, hidden=D, ensemble=3)
    B, rates, DEAD = 2 * mb, (0.2, 0.3), D - 3
    trunk, theta = O.init_params(cfg, 42)
    st = O.TrainState(cfg, trunk, theta, torch.float64)
    core = AH.load_leaves(_core(cfg, B, rates, fuse), cfg, None, theta)
    b, noise = AH.synth_batch(cfg, B, seed=3), O.make_noise(cfg, B, seed=7, utd_ratio=2)
    masks = MD.random_masks(rates, "high_utd", 2, (), B, D, seed=11)
    assert set(masks) == set(MD.MLP_SITES)
    for m in masks.values():
        m[:, :, DEAD] = 0
    crit_grads, cu = [], O.critic_update

    def recording(*a, **k):
        info, aux = cu(*a, **k)
        crit_grads.append(aux["grads"])
        return info, aux
    O.critic_update = recording
    try:
        with MD.oracle_dropout(rates, MD.mask_queue(masks, rates, "high_utd", 2, (), B)):
            info, aux = O.update_high_utd(st, AH.batch_to_torch(b, torch.float64), O.noise_to_torch(noise, torch.float64), 2)
    finally:
        O.critic_update = cu
    core.update_high_utd(AH.batch_to_device(cfg, b), 2, {**AH.noise_to_device(cfg, noise), **MD.device_noise(masks)})
    fig = _Figures(f"dropout rows w{D} mb{mb} fuse={fuse}")
    _info(fig, core.read_info(), info, ("critic_loss", "predicted_qs", "target_qs", "actor_loss", "temperature", "entropy", "temperature_loss"))
    _grads(fig, cfg, core, crit_grads[-1], "g_critic")
    _grads(fig, cfg, core, aux["g_actor"], "g_actor")
    # exact zeros: the dropped column of both layers, critic (three groups, rows mb.. of the masks) and policy (one group)
    sl, _ = AH.leaf_slices(cfg)
    gc = core.debug("g_critic", sl["critic/head/bias"][1])
    lo0 = sl["actor/w1"][0]
    ga = core.debug("g_actor", sl["actor/logstd/bias"][1] - lo0)
    for net, g, off in (("critic", gc, 0), ("actor", ga, lo0)):
        for j in (1, 2):
            w, bias = g[sl[f"{net}/w{j}"][0] - off:sl[f"{net}/w{j}"][1] - off], g[sl[f"{net}/b{j}"][0] - off:sl[f"{net}/b{j}"][1] - off]
            assert not w.reshape(-1, D)[:, DEAD].any() and not bias.reshape(-1, D)[:, DEAD].any(), (net, j)
            assert np.abs(w.reshape(-1, D)[:, :DEAD]).max() > 0 and np.abs(bias.reshape(-1, D)[:, DEAD - 1]).max() > 0
    # the policy's backward ran last: the gradient wrt its Dense outputs is exactly 0 where "pi" dropped and nowhere else, and
    # the dropped inputs of a LayerNorm row are one value (the row's normalised 0)
    for layer in (1, 2):
        keep = masks["pi"][layer - 1].astype(bool)
        dpre = core.debug(f"mlp_dpre/{layer}", B * D).reshape(B, D)
        assert not dpre[~keep].any() and dpre[keep].all(), layer
        xhat = core.debug(f"mlp_xhat/pol__/{layer}", B * D).reshape(B, D)
        for r in range(B):
            assert np.unique(xhat[r][~keep[r]]).size == 1, (layer, r)
    fig.check()
    _compare_state(cfg, st, core, steps=3)
    assert core.step == st.step == 3 and core.debug("ctr_nonzero", 1)[0] == 0


# ---- evaluation --------------------------------------------------------------------------------------------------------------------
def test_evaluate_losses_with_the_fixtures_noise_is_the_updates_info(gpu):
    agent, g, _ = _fixture_agent("update_sac_state")
    cfg = g["cfg"]
    step = g["steps"][1]
    assert step["kind"] == "update"
    noise = AH.noise_to_device(cfg, {k: (v.astype(np.float32) if k.startswith("eps") else v) for k, v in step["noise"].items()})
    noise.update(MD.device_noise(MD.unpack(step["noise"], g["B"], cfg.hidden)))
    batch = GR.ref_batch(cfg, step["batch"], unpacked=True)
    before = _bits(agent.core)
    dry = agent.evaluate_losses(batch, noise=dict(noise))
    _same_bits(_bits(agent.core), before, "evaluate_losses wrote the state")
    plain = agent.evaluate_losses(batch, noise={k: v for k, v in noise.items() if not k.startswith("drop_")})
    _, info = agent.update(batch, noise=dict(noise))
    for net in ("critic", "actor", "temperature"):
        assert dry[net] == {k: info[net][k] for k in dry[net]}, (net, dry[net], info[net])
    assert plain["critic"]["critic_loss"] != dry["critic"]["critic_loss"]      # (hashed masks instead: another loss)


def test_evaluation_calls_ignore_the_rates_and_write_nothing(gpu):
    S, A, B, h = 10, 5, 72, 256
    cfg = O.Config(image_keys=(), S=S, A=A, discount=0.99, hidden=h)
    theta = O.init_params(cfg, GR.PARAM_SEED)[1]
    import mlp_widths as MW
    drop = MW.sac_agent(h, seed=3, B=B, S=S, A=A, critic_network_kwargs=MD.network_kwargs(cfg, "critic", 0.3),
                        policy_network_kwargs=MD.network_kwargs(cfg, "policy", 0.4), mlp_dropout=True)
    plain = MW.sac_agent(h, seed=3, B=B, S=S, A=A)
    for a in (drop, plain):
        AH.load_leaves(a.core, cfg, None, theta)
    assert drop.core.critic_dropout == 0.3 and plain.core.critic_dropout == 0.0
    rng = np.random.default_rng(6)
    state, act = rng.standard_normal((B, S)).astype(np.float32), rng.uniform(-0.9, 0.9, (B, A)).astype(np.float32)
    before = _bits(drop.core)
    seed = np.array([0, 11], np.uint32)
    for target in (False, True):
        assert np.array_equal(drop.q_values(state, act, target=target), plain.q_values(state, act, target=target))
    ps, pp = drop.policy_stats(state, act), plain.policy_stats(state, act)
    assert set(ps) == set(pp) and all(np.array_equal(ps[k], pp[k]) for k in ps)
    assert np.array_equal(drop.sample_actions(state, argmax=True), plain.sample_actions(state, argmax=True))
    assert np.array_equal(drop.sample_actions(state, seed=seed), plain.sample_actions(state, seed=seed))
    _same_bits(_bits(drop.core), before, "an evaluation call wrote the state")


def test_rate_zero_through_create_dropout_is_create_mlp_bit_for_bit(gpu):
    from serl_amd.agents.core import AgentCore

    class OldEntry(AgentCore):
        def _create(self, cfg):
            return self.L.serl_agent_create_mlp(C.byref(cfg), self._std_param, 0 if self.tanh_squash_distribution else 1, *self._acts,
                                                C.byref(self._h))
    for hidden in (256, 192):
        cfg, B = O.Config(image_keys=(), S=10, A=3, discount=0.99, hidden=hidden), 72
        _, theta = O.init_params(cfg, 42)
        kw = dict(encoder_type=cfg.encoder_type, n_cam=0, H=0, W=0, state_dim=cfg.S, act_dim=cfg.A, batch=B, ensemble=cfg.ensemble,
                  hidden=hidden, discount=cfg.discount, tau=cfg.tau, lr=cfg.lr, warmup_steps=cfg.warmup, dropout=cfg.dropout,
                  std_min=cfg.std_min, std_max=cfg.std_max, target_entropy=cfg.target_entropy, seed=5, temp_warmup_steps=-1)
        old, new = OldEntry(**kw), AgentCore(critic_dropout=0.0, policy_dropout=0.0, **kw)
        b, noise = AH.synth_batch(cfg, B, seed=5), O.make_noise(cfg, B, seed=9, utd_ratio=2)
        for core in (old, new):
            AH.load_leaves(core, cfg, None, theta)
            core.update_high_utd(AH.batch_to_device(cfg, b), 2, AH.noise_to_device(cfg, noise))      # injected draws
            core.update_high_utd(AH.batch_to_device(cfg, b), 2)                                         # the device hash from cfg.seed
        assert old.step == new.step == 6 and old.read_info() == new.read_info()
        _same_bits(_bits(new), _bits(old), f"hidden {hidden}")


def test_positive_rates_through_create_dropout_are_create_opts_bit_for_bit(gpu):
    """the same comparison at rate 0.5 in both networks: serl_agent_create_dropout fills the struct AgentCore hands to
    serl_agent_create_opts.  Explicit keep-masks, so both agents see the same draws."""
    from serl_amd.agents.core import AgentCore

    class OldEntry(AgentCore):
        def _create(self, cfg):
            return self.L.serl_agent_create_dropout(C.byref(cfg), self._std_param, 0 if self.tanh_squash_distribution else 1, *self._acts,
                                                    self.critic_dropout, self.policy_dropout, C.byref(self._h))
    cfg, B, rates = O.Config(image_keys=(), S=10, A=4, discount=0.99, hidden=64, ensemble=2), 8, (0.5, 0.5)
    _, theta = O.init_params(cfg, 42)
    kw = dict(encoder_type=cfg.encoder_type, n_cam=0, H=0, W=0, state_dim=cfg.S, act_dim=cfg.A, batch=B, ensemble=cfg.ensemble,
              hidden=cfg.hidden, discount=cfg.discount, tau=cfg.tau, lr=cfg.lr, warmup_steps=cfg.warmup, dropout=cfg.dropout,
              std_min=cfg.std_min, std_max=cfg.std_max, target_entropy=cfg.target_entropy, seed=5, temp_warmup_steps=-1,
              critic_dropout=rates[0], policy_dropout=rates[1])
    old, new = OldEntry(**kw), AgentCore(**kw)
    assert list(old.leaves.items()) == list(new.leaves.items())
    b = AH.synth_batch(cfg, B, seed=5)
    n1, n2 = O.make_noise(cfg, B, seed=8), O.make_noise(cfg, B, seed=9, utd_ratio=2)
    m1, m2 = MD.random_masks(rates, "critics", 1, (), B, cfg.hidden, seed=11), MD.random_masks(rates, "high_utd", 2, (), B, cfg.hidden, seed=12)
    assert set(m2) == set(MD.MLP_SITES)
    for core in (old, new):
        AH.load_leaves(core, cfg, None, theta)
        core.update_critics(AH.batch_to_device(cfg, b), {**AH.noise_to_device(cfg, n1), **MD.device_noise(m1)})
        core.update_high_utd(AH.batch_to_device(cfg, b), 2, {**AH.noise_to_device(cfg, n2), **MD.device_noise(m2)})
    assert old.step == new.step > 0 and old.read_info() == new.read_info()
    _same_bits(_bits(new), _bits(old), "rates 0.5")


def test_c_abi_refuses_rates_outside_the_unit_interval(gpu):
    from serl_amd import _lib
    from serl_amd._lib_agent import SerlAgentCfg
    L = _lib.lib()
    cfg = SerlAgentCfg(0, 0, 0, 0, 10, 4, 8, 10, 256, 256, 8, 64, 0, -1, 0.99, 0.005, 3e-4, 0.1, 1e-5, 5.0, -2.0, 0)
    for rates, which in (((1.0, 0.0), "critic_dropout"), ((0.0, -0.1), "policy_dropout"), ((2.0, 0.5), "critic_dropout")):
        h = C.c_void_p()
        rc = int(L.serl_agent_create_dropout(C.byref(cfg), 0, 0, 0, 0, *rates, C.byref(h)))
        assert rc == -1 and which in (L.serl_last_error() or b"").decode() and "[0, 1)" in (L.serl_last_error() or b"").decode()
    h = C.c_void_p()
    assert int(L.serl_agent_create_dropout(C.byref(cfg), 0, 0, 0, 0, 0.5, 0.99, C.byref(h))) == 0 and int(L.serl_agent_destroy(h)) == 0


# ---- data-parallel shards ----------------------------------------------------------------------------------------------------------
def _half(b, r, n):
    return {k: ({} if isinstance(v, dict) else v[r * n:(r + 1) * n]) for k, v in b.items()}


@pytest.mark.parametrize("stream", ["keys", "hash"])
def test_two_shards_of_a_batch_equal_the_full_batch(gpu, stream):
    """tests/test_agent_gpu.py::test_dp_split_equals_full_batch with MLP Dropout: a rank draws (or hashes) its rows of the global masks"""
    from serl_amd.call_noise import CallNoise
    cfg = O.Config(image_keys=(), S=10, A=3, discount=0.99, hidden=192, ensemble=3)
    B, rates = 16, (0.2, 0.25)
    _, theta = O.init_params(cfg, 42)
    b = AH.synth_batch(cfg, B, seed=5)
    sl, _ = AH.leaf_slices(cfg)
    n, lo0 = sl["critic/head/bias"][1], sl["actor/w1"][0]
    na = sl["actor/logstd/bias"][1] - lo0
    keys = J.UpdateKeys(J.prngkey(9), False, 1, True, False, False)

    def run(rows, shard):
        core = AH.load_leaves(_core(cfg, rows, rates, agent_seed=7), cfg, None, theta)
        if shard is not None:
            core.set_shard(shard * rows, B)
        noise = (lambda **w: CallNoise(core, (), {}).build(keys, rows, "keys", **w)) if stream == "keys" else (lambda **w: None)
        db = AH.batch_to_device(cfg, b if shard is None else _half(b, shard, rows))
        core.begin_update()
        core.encode(db)
        core.critic_grads(0, rows, B, noise(want_actor=False))
        gc, sc = core.debug("g_critic", n).astype(np.float64), core.debug("scalars", 3).astype(np.float64)
        core.actor_grads(B, noise(want_critic=False))
        return gc, sc, core.debug("g_actor", na).astype(np.float64)
    full = run(B, None)
    parts = [run(B // 2, r) for r in range(2)]
    for i, what in enumerate(("g_critic", "scalars", "g_actor")):
        err = AH.rel_err(parts[0][i] + parts[1][i], full[i])
        print(f"{stream}: two shards vs the full batch, {what}: {err:.2e}")
        assert np.abs(full[i]).max() > 0 and err < 1e-5, what


# ---- the hash stream ---------------------------------------------------------------------------------------------------------------
def _dropped(xhat):
    """[rows, D] normalised LayerNorm inputs -> bool [rows, D]: the elements that carry the row's most frequent value, the
    normalised 0 of the dropped ones (at keep 0.9 and D = 256 a row without two dropped elements has probability 1e-10)"""
    out = np.zeros(xhat.shape, bool)
    for r, row in enumerate(xhat):
        v, c = np.unique(row, return_counts=True)
        assert c.max() >= 2, r
        out[r] = row == v[c.argmax()]
    return out


def test_hash_stream_keeps_the_rate_and_agrees_forward_and_backward(gpu):
    cfg = O.Config(image_keys=(), S=10, A=5, discount=0.99, hidden=256, ensemble=3)
    B, D, E, keep = 72, 256, 3, 0.9
    core = AH.load_leaves(_core(cfg, B, (1 - keep, 1 - keep), agent_seed=4), cfg, None, O.init_params(cfg, 42)[1])
    db = AH.batch_to_device(cfg, AH.synth_batch(cfg, B, seed=3))
    bound = 6 * np.sqrt(B * D * keep * (1 - keep))      # 6 binomial standard deviations of n = rows * D draws: 244 of 18432
    seen = {}

    def site(name, buf, members, backward):
        for layer in (1, 2):
            x = core.debug(f"mlp_xhat/{buf}/{layer}", members * B * D).reshape(members, B, D)
            drop = _dropped(x[0])
            for m in range(1, members):      # one mask for every member
                assert np.array_equal(_dropped(x[m]), drop), (name, layer, m)
            kept = int((~drop).sum())
            print(f"hash {name} layer {layer}: kept {kept} of {B * D} ({kept / (B * D):.4f})")
            assert abs(kept - keep * B * D) <= bound, (name, layer, kept)
            if backward:
                dpre = core.debug(f"mlp_dpre/{layer}", members * B * D).reshape(members, B, D)
                for m in range(members):
                    assert np.array_equal(dpre[m] == 0, drop), (name, layer, m)
            seen[(name, layer)] = drop
    core.begin_update()
    core.encode(db)
    core.critic_grads(0, B, B)
    site("pi_next", "pol__", 1, False)
    site("q_target", "critT", E, False)
    site("q_online", "crit_", E, True)
    core.actor_grads(B)
    site("pi_temp", "polT_", 1, False)
    site("q_actor", "crit_", E, False)
    site("pi", "pol__", 1, True)
    masks = list(seen.values())      # a stream per (site, layer)
    assert all(not np.array_equal(masks[i], masks[j]) for i in range(len(masks)) for j in range(i))
