"""GPU: weight_decay in the optimizer kwargs of an agent with cameras (serl_mi355.h, LIVE TRUNK; serl_amd/csrc/agent.hip
live_features).  adamw decays the whole tree, the pretrained ResNet-10 included: the online trunk shrinks at every optimizer
step, the target copy follows by the EMA, the target critic reads features of the target copy, and the features are recomputed
after every step.

* creation succeeds, pretrained (live_trunk) and SmallEncoder (not live: no frozen leaf);
* the reference's own runs (tests/golden/wd_*.npz) through tests/golden_replay.py::replay at its TOL, the pretrained ones in both
  trunk modes, and once on an agent whose batch capacity exceeds the rows (every pass then takes the partial-batch path; at
  capacity == rows update_critics and the actor phase take the contiguous pass, the 3-row minibatches the partial one);
* every trunk leaf, online and target, after the schedule against the float64 oracle (TrainState.live_trunk),
  element by element: |got - ref| <= 1e-4 |p0 - ref| + 2 n ulp(p0) -- tests/test_optimizer_layouts_gpu.py's bound for one step
  (optimizer_cases.STEP_REL of the step, 2 ulp of the parameter), summed over the n steps of a monotone decay; a target element
  is an average of online values with weights that sum to 1 and rounds twice more per EMA step: 2 n_ema ulp(p0) on top;
* q_values(target=True) and sample_actions(argmax=True) after the schedule against the restatement, at TOL;
* evaluate_losses reports the scalars of the update that follows, bit for bit, and neither it nor q_values changes that update;
* a checkpoint with a decayed trunk restores bit for bit, and the next update is identical;
* reward labels come from the classifier's own trunk ("frames") although the trunks are equal at the attach, over two labelled
  updates, with no "attach again" error after the optimizer changed the trunk;
* DataParallelLearner, one rank, serial schedule: the agent's bytes;
* decay 0 in all three optimizers, through the same kwargs: not live, and byte-identical to an agent created without them.
"""
import functools
import itertools

import numpy as np
import pytest
import torch

from helpers import make_spaces
from oracle import drq_oracle as O
import agent_helpers as AH
import golden_replay as GR
import mlp_widths as MW
import optimizer_cases as OC
import pixel_weight_decay as PW
from test_agent_gpu import _compare_state
from test_mlp_widths_gpu import _Figures, _grads, _info
from test_pixel_weight_decay_cpu import _restated

pytestmark = pytest.mark.gpu
TOL = GR.TOL
SECTIONS = ("params", "target_params", "opt/critic/mu", "opt/critic/nu", "opt/actor/mu", "opt/actor/nu", "opt/temperature/mu",
            "opt/temperature/nu")


def _identity(theta, cfg):
    return {k: np.array(v, np.float32) for k, v in theta.items()}


def _agent(cfg, B, trunk_mode=None, **kw):
    """DrQAgent.create_drq as the launcher calls it, with the Config's optimizer kwargs, holding O.init_params' leaves"""
    agent = GR.reference_agent(cfg, B, **kw)
    if trunk_mode is not None:
        agent.core.set_trunk_mode(trunk_mode)
    AH.load_leaves(agent.core, cfg, *GR.initial_leaves(cfg, _identity))
    return agent


@functools.lru_cache(maxsize=None)
def _replayed(name, trunk_mode, capacity=None):
    """the agent after the recorded schedule of wd_<name>.npz (GR.replay's own comparisons on the way), once per session"""
    g = _restated(name)[0]
    agent = _agent(g["cfg"], capacity or g["B"], trunk_mode)
    assert agent.live_trunk == (not g["cfg"].small) and agent.core.live_trunk == agent.live_trunk
    GR.replay(agent, g, label=f"wd_{name} {trunk_mode} capacity {capacity or g['B']}")
    assert agent.core.debug("ctr_nonzero", 1)[0] == 0
    return agent


def _bits(core):
    return {(sec, leaf): core.get(sec, leaf).copy() for leaf in core.leaves for sec in SECTIONS
            if not (leaf.startswith("trunk/") and sec.startswith("opt/"))}


def _assert_same_bits(got, want, what):
    assert set(got) == set(want)
    for key, v in got.items():
        assert np.array_equal(v.view(np.uint32), want[key].view(np.uint32)), (what, key)


# ---- creation --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["update_drq_one_cam", "update_drq_small"])
def test_weight_decay_on_a_pixel_agent_is_accepted(gpu, name):
    cfg, B = PW.GOLDEN[name][0], PW.GOLDEN[name][1]
    agent = _agent(cfg, B)
    assert agent.live_trunk == (not cfg.small)
    assert agent.state.opt_states["critic"]["hyperparams"]["weight_decay"] == np.float32(PW.DECAY["critic"])


# ---- the reference's own runs ----------------------------------------------------------------------------------------------------
REPLAYS = [("update_drq_one_cam", "f16x3", None), ("update_drq_one_cam", "f32", None), ("update_drq_one_cam", "f16x3", 8),
           ("update_sac_pixels_update", "f16x3", None), ("update_sac_pixels_update", "f32", None), ("update_drq_small", None, None)]


@pytest.mark.parametrize("name,trunk_mode,capacity", REPLAYS, ids=[f"{n}-{m}-{c}" for n, m, c in REPLAYS])
def test_hip_update_matches_the_reference_golden_with_weight_decay(gpu, name, trunk_mode, capacity):
    _replayed(name, trunk_mode, capacity)


PRETRAINED = [r for r in REPLAYS if r[0] in PW.PRETRAINED]


@pytest.mark.parametrize("name,trunk_mode,capacity", PRETRAINED, ids=[f"{n}-{m}-{c}" for n, m, c in PRETRAINED])
def test_every_trunk_leaf_matches_the_restatement(gpu, name, trunk_mode, capacity):
    g, _, st, _ = _restated(name)
    core = _replayed(name, trunk_mode, capacity).core
    trunk0, _ = O.init_params(g["cfg"], g["meta"]["param_seed"])
    _check_trunk_leaves(core, st, trunk0, PW.optimizer_steps(PW.GOLDEN[name][2]), f"wd_{name} {trunk_mode} capacity {capacity}")


def _check_trunk_leaves(core, st, trunk0, steps, label):
    """every trunk leaf of the agent, online and target, against the oracle's after `steps` (PW.optimizer_steps), element by
    element, with the bound of the module docstring"""
    n, n_ema = len(steps), sum(steps)
    worst = {"params": 0.0, "target_params": 0.0}
    for k, v0 in trunk0.items():
        p0 = v0.astype(np.float64).reshape(-1)
        ref_on = st.trunk[k].numpy().reshape(-1)
        moved = OC.STEP_REL * np.abs(p0 - ref_on) + 2.0 * n * OC.ulp(p0)
        for sec, ref, bound in (("params", ref_on, moved),
                                ("target_params", st.target_trunk[k].numpy().reshape(-1), moved + 2.0 * n_ema * OC.ulp(p0))):
            got = core.get(sec, k).astype(np.float64)
            err = np.abs(got - ref)
            nz = bound > 0
            assert (err[~nz] == 0).all(), (sec, k)
            i = int(np.argmax(err[nz] / bound[nz])) if nz.any() else 0
            worst[sec] = max(worst[sec], float((err[nz] / bound[nz]).max()) if nz.any() else 0.0)
            assert (err <= bound).all(), (sec, k, i, got[nz][i], ref[nz][i], err[nz][i], bound[nz][i])
        assert (np.abs(core.get("params", k)) <= 0.95 * np.abs(v0.reshape(-1))).all(), k      # the trunk did decay
    print(f"{label}: trunk leaves, worst err / bound: online {worst['params']:.3f}, target {worst['target_params']:.3f}")


@pytest.mark.parametrize("name,trunk_mode,capacity", PRETRAINED[:2], ids=[f"{n}-{m}-{c}" for n, m, c in PRETRAINED[:2]])
def test_read_paths_use_the_right_trunk(gpu, name, trunk_mode, capacity):
    """forward_target_critic runs the target copy of the trunk, the policy the online one: both against the restatement, and far
    from what the other trunk gives"""
    g, _, st, _ = _restated(name)
    cfg = g["cfg"]
    agent = _replayed(name, trunk_mode, capacity)
    pb = g["steps"][0]["batch"]
    frames = {k: v[:, 0] for k, v in pb["frames"].items()}
    state, action = pb["state"][:, 0], pb["action"]
    obs = {**frames, "state": state[:, None]}
    ft = {k: torch.from_numpy(v) for k, v in frames.items()}
    s64, a64 = torch.tensor(state, dtype=torch.float64), torch.tensor(action, dtype=torch.float64)
    with torch.no_grad():
        q = {}
        for which, params, target in (("target", st.target, True), ("online", st.params, False), ("target on online trunk", st.target, False)):
            q[which] = O.critic_forward(params, cfg, O.encode(params, cfg, O.features(st, ft, target=target), s64), a64).numpy()
        mean, _ = O.policy_head(st.params, cfg, O.encode(st.params, cfg, O.features(st, ft), s64))
        mean_t, _ = O.policy_head(st.params, cfg, O.encode(st.params, cfg, O.features(st, ft, target=True), s64))
    e_t = AH.rel_err(agent.q_values(obs, action, target=True), q["target"])
    e_o = AH.rel_err(agent.q_values(obs, action), q["online"])
    e_m = AH.rel_err(agent.sample_actions(obs, argmax=True), torch.tanh(mean).numpy())
    apart_q, apart_m = AH.rel_err(q["target on online trunk"], q["target"]), AH.rel_err(torch.tanh(mean_t).numpy(), torch.tanh(mean).numpy())
    print(f"wd_{name} {trunk_mode}: q_values target {e_t:.2e}, online {e_o:.2e}, mode {e_m:.2e}; the other trunk would be "
          f"{apart_q:.2e} (Q) and {apart_m:.2e} (mode) away")
    assert apart_q > 100 * TOL and apart_m > 100 * TOL      # (a condition on the fixture: the comparison can tell the trunks apart)
    assert e_t < TOL and e_o < TOL and e_m < TOL


# ---- every option at once -------------------------------------------------------------------------------------------------------
def test_all_options_at_once_match_the_oracle(gpu):
    """PW.COMPOSED -- softplus std, swish in both MLPs, the decay on a pretrained trunk -- in one serl_agent_create_mlp call against
    the one oracle: update_critics (6 rows = the agent's capacity) then update_high_utd(2) (3-row minibatches: the partial-batch
    path), with the comparisons and bounds of tests/test_mlp_activations_gpu.py::_compare_rows and, for the trunk leaves, of
    test_every_trunk_leaf_matches_the_restatement"""
    cfg, B = PW.COMPOSED, PW.COMPOSED_ROWS
    trunk0, theta = O.init_params(cfg, GR.PARAM_SEED)
    st = O.TrainState(cfg, trunk0, theta, torch.float64)
    core = AH.load_leaves(AH.make_core(cfg, B), cfg, trunk0, theta)
    assert st.live_trunk and core.live_trunk and core.std_parameterization == "softplus"
    assert (core.critic_activation, core.policy_activation) == ("swish", "swish")
    b1, n1 = AH.synth_batch(cfg, B, seed=3), O.make_noise(cfg, B, seed=7)
    b2, n2 = AH.synth_batch(cfg, B, seed=4), O.make_noise(cfg, B, seed=8, utd_ratio=2)
    info1, aux1 = O.update_critics(st, AH.batch_to_torch(b1, torch.float64), O.noise_to_torch(n1, torch.float64))
    info2, aux2 = O.update_high_utd(st, AH.batch_to_torch(b2, torch.float64), O.noise_to_torch(n2, torch.float64), 2)
    fig = _Figures("composed softplus / swish / decay")
    core.update_critics(AH.batch_to_device(cfg, b1), AH.noise_to_device(cfg, n1))
    _info(fig, core.read_info(), info1, ("critic_loss", "predicted_qs", "target_qs"))
    fig.add("q", AH.rel_err(core.debug("q", cfg.ensemble * B).reshape(cfg.ensemble, B), aux1["q"].numpy()))
    fig.add("target_q", AH.rel_err(core.debug("target_q", B), aux1["target_q"].numpy()))
    fig.add("next logp", AH.rel_err(core.debug("logp", B), aux1["next_logp"].numpy()))
    _grads(fig, cfg, core, aux1["grads"], "g_critic")
    core.update_high_utd(AH.batch_to_device(cfg, b2), 2, AH.noise_to_device(cfg, n2))
    _info(fig, core.read_info(), info2,
          ("critic_loss", "predicted_qs", "target_qs", "actor_loss", "temperature", "entropy", "temperature_loss"))
    _grads(fig, cfg, core, aux2["g_actor"], "g_actor")
    fig.check()
    _compare_state(cfg, st, core, steps=4)
    assert core.step == st.step == 4
    _check_trunk_leaves(core, st, trunk0, PW.optimizer_steps([("critics",), ("high_utd", 2)]), "composed")
    assert core.debug("ctr_nonzero", 1)[0] == 0


# ---- checkpoints -----------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip_with_a_decayed_trunk(gpu, tmp_path):
    from serl_amd.utils.checkpoint import restore_checkpoint, save_checkpoint
    name = "update_drq_one_cam"
    g = _restated(name)[0]
    cfg, B = g["cfg"], g["B"]
    agent = _agent(cfg, B)
    step = g["steps"][1]
    noise = AH.noise_to_device(cfg, {k: (v.astype(np.float32) if k.startswith("eps") else v) for k, v in step["noise"].items()
                                     if not k.startswith("crop")})
    crops = (step["noise"]["crop_obs"].astype(np.int32), step["noise"]["crop_next"].astype(np.int32))
    agent.update_high_utd(GR.ref_batch(cfg, step["batch"]), utd_ratio=2, noise=noise, crops=crops)
    save_checkpoint(str(tmp_path / "wd"), agent, step=agent.state.step)
    fresh = _agent(cfg, B)
    restore_checkpoint(str(tmp_path / "wd"), fresh, restore_rng=True)
    assert fresh.state.step == agent.state.step == 3
    want = _bits(agent.core)
    trunk0, _ = O.init_params(cfg, GR.PARAM_SEED)
    assert not np.array_equal(want[("params", "trunk/conv_init")], trunk0["trunk/conv_init"].reshape(-1))
    assert not np.array_equal(want[("params", "trunk/conv_init")], want[("target_params", "trunk/conv_init")])
    _assert_same_bits(_bits(fresh.core), want, "restored")
    for a in (agent, fresh):
        a.update_high_utd(GR.ref_batch(cfg, step["batch"]), utd_ratio=2, noise=noise, crops=crops)
    assert agent.core.read_info() == fresh.core.read_info()
    _assert_same_bits(_bits(fresh.core), _bits(agent.core), "after the next update")


# ---- read-only evaluation --------------------------------------------------------------------------------------------------------
def test_evaluate_losses_is_the_next_update_and_leaves_it_alone(gpu):
    """loss_fns(batch) on a live trunk: the target critic's side through the target copy, in the scratch slot -- the scalars are
    those of the update that follows, bit for bit, and that update leaves the bytes it leaves without the evaluation"""
    cfg, B = PW.GOLDEN["update_drq_one_cam"][0], 6
    b1, n1 = AH.synth_batch(cfg, B, seed=3), O.make_noise(cfg, B, seed=7, utd_ratio=2)
    b2, n2 = AH.synth_batch(cfg, B, seed=4), O.make_noise(cfg, B, seed=8, utd_ratio=1)
    out = []
    for evaluate in (True, False):
        agent = _agent(cfg, B)
        agent.update_high_utd(AH.batch_to_device(cfg, b1), utd_ratio=2, noise=AH.noise_to_device(cfg, n1))      # the trunks differ now
        db, dn = AH.batch_to_device(cfg, b2), AH.noise_to_device(cfg, n2)
        dry = agent.evaluate_losses(db, noise=dn) if evaluate else None
        q_t = agent.q_values({"image": b2["next"]["image"], "state": b2["next_state"][:, None]}, b2["action"], target=True) if evaluate else None
        _, info = agent.update(db, noise=dn)
        out.append((dry, q_t, info.resolve(), _bits(agent.core)))
    (dry, _, info, bits), (_, _, info_plain, bits_plain) = out
    assert dry == info == info_plain, (dry, info, info_plain)
    _assert_same_bits(bits, bits_plain, "an update behind evaluate_losses and q_values")


# ---- reward labels ---------------------------------------------------------------------------------------------------------------
def test_reward_labels_come_from_the_classifiers_own_trunk(gpu):
    import test_reward_labels_gpu as RL
    c = RL._case()                      # classifier seed 42: its trunk equals the agent's at the attach
    cfg = O.Config(opt=PW.OPT, **{k: getattr(c["cfg"], k) for k in ("image_keys", "H", "W", "S", "A")})
    B = c["labels"].size
    live, frozen = _agent(cfg, B), _agent(c["cfg"], B)
    frozen.set_reward_classifier(RL._classifier(c))
    assert frozen.reward_label_mode == "features" and not frozen.live_trunk
    live.set_reward_classifier(RL._classifier(c))
    assert live.live_trunk and live.reward_label_mode == "frames"
    db, dn = AH.batch_to_device(cfg, c["b"]), AH.noise_to_device(cfg, c["noise"])
    live.update_critics(db, noise=dn)
    RL._check_labels(live, c)
    _, pending = live.update_high_utd(db, utd_ratio=1, noise=dn)      # the optimizer has changed the trunk: no "attach again"
    RL._check_labels(live, c)
    assert abs(pending.resolve()["vice_rewards"] - float(c["labels"].mean())) <= 2 ** -22
    assert live.core.step == 3


# ---- the learner -----------------------------------------------------------------------------------------------------------------
KEYS, H, W, S, A, SEED = ("image",), 64, 64, 5, 3, 3


def _store():
    from serl_amd.data.data_store import MemoryEfficientReplayBufferDataStore
    from serl_amd.utils.synthetic import transition_stream
    osp, asp = make_spaces(KEYS, H, W, 3, 1, S, A)
    rb = MemoryEfficientReplayBufferDataStore(osp, asp, 200, image_keys=KEYS)
    rb.seed(0)
    for tr in itertools.islice(transition_stream(KEYS, H, W, 3, 1, S, A, 20, 1), 120):
        rb.insert(tr)
    return rb


def _decay_kwargs(decay):
    return {f"{tx}_optimizer_kwargs": {"weight_decay": wd} for tx, wd in decay.items()}


def _seeded_agent(B, **kw):
    return MW.drq_agent(256, KEYS, H, W, S, A, seed=SEED, B=B, **kw)


def _end_state(core, rng):
    torch.cuda.synchronize()
    return {"rng": np.array(rng), "step": core.step, "bits": _bits(core)}


def _run_agent(B, **kw):
    agent, rb = _seeded_agent(B, **kw), _store()
    it = rb.get_iterator(sample_args={"batch_size": B, "pack_obs_and_next_obs": True, "lazy": True})
    for _ in range(2):
        agent.update_critics(next(it))
        agent.update_high_utd(next(it), utd_ratio=1)
    return agent, _end_state(agent.core, agent.state.rng)


def test_data_parallel_learner_one_rank_equals_the_agent(gpu):
    from serl_amd.agents.batch import DeviceBatch
    from serl_amd.data.data_store import gather_crop
    from serl_amd.parallel import DataParallelLearner, SerialSchedule, TorchPipelineSchedule, TrunkFarmLearner
    B = 6
    agent, a = _run_agent(B, **_decay_kwargs(PW.DECAY))
    assert agent.live_trunk and agent._sched is None      # prefetch is on and has no effect: nothing ran on a side stream
    core, rb, dbs = _seeded_agent(B, **_decay_kwargs(PW.DECAY)).core, _store(), {}

    def gather(parts, co, cn, slot):
        if slot not in dbs:
            dbs[slot] = DeviceBatch(B, len(KEYS), H, W, 3, S, A, 0)
        gather_crop(parts, co, cn, dbs[slot])
        return dbs[slot]

    with pytest.raises(ValueError, match="live"):
        DataParallelLearner(core, gather, [rb], [B], seed=SEED, image_keys=KEYS, device_noise="threefry",
                            schedule=TorchPipelineSchedule(core.device))
    with pytest.raises(NotImplementedError, match="live"):
        TrunkFarmLearner(core, gather, [rb], [B], rank=0, world=2, seed=SEED)
    lr = DataParallelLearner(core, gather, [rb], [B], seed=SEED, image_keys=KEYS, device_noise="threefry", schedule=SerialSchedule())
    for _ in range(2):
        lr.iteration(2)
    l = _end_state(core, lr._rng)
    assert np.array_equal(a["rng"], l["rng"]) and a["step"] == l["step"] == 6
    _assert_same_bits(l["bits"], a["bits"], "learner vs agent")
    on, tg = a["bits"][("params", "trunk/conv_init")], a["bits"][("target_params", "trunk/conv_init")]
    assert not np.array_equal(on, tg)


# ---- no decay, no change ---------------------------------------------------------------------------------------------------------
def test_zero_decay_is_the_frozen_trunk_bit_for_bit(gpu):
    B = 6
    zero, z = _run_agent(B, **_decay_kwargs({tx: 0.0 for tx in PW.DECAY}))
    plain, p = _run_agent(B)
    assert not zero.live_trunk and not plain.live_trunk
    assert zero.state.opt_states["actor"]["hyperparams"]["weight_decay"] == np.float32(0.0)
    assert "weight_decay" not in plain.state.opt_states["actor"]["hyperparams"]
    assert np.array_equal(z["rng"], p["rng"]) and z["step"] == p["step"] == 6
    _assert_same_bits(z["bits"], p["bits"], "decay 0 vs no decay")
