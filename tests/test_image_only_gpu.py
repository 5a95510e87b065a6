"""GPU: agents without the proprio branch (serl_agent_opts.no_proprio; create_drq(image_only=True, use_proprio=False)) under the
whole update chain, on the case table of tests/image_only.py.

* oracle parity of update_critics and update_high_utd in both schedules of the chain, with injected noise: info scalars, q,
  target_q, next log-prob, every gradient leaf and the state after the step at the tolerances of tests/test_mlp_plain_gpu.py
  (TOL = 1e-4, _compare_state).  update_high_utd runs at utd_ratio 2 where 2 divides the rows, else at the smallest divisor above 1
  (5 at 65 rows), and at 1 on one row: the reference asserts that the ratio divides the batch;
* the actions rider, the state never read (NaN states, NULL state pointers), the default agent untouched (bits and launch counts),
  the launch count against the proprio twin, a cross-check against a proprio agent whose proprio rows of the first kernels are zero,
  the read-only calls, checkpoints, snapshots, reward labels and two shards."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import classifier_oracle as CO
from oracle import drq_oracle as O
import agent_helpers as AH
import image_only as IO
import mlp_ragged as MR
import stacked_oracle as SO
from test_agent_gpu import TOL, _compare_state
from test_chain_fusion_gpu import _bits_equal, _launches
from test_evaluate_gpu import _same, _state_of
from test_mlp_widths_gpu import _Figures, _info

pytestmark = pytest.mark.gpu
FUSE = pytest.mark.parametrize("fuse", [True, False], ids=["fused", "unfused"])


@pytest.fixture(autouse=True)
def _general_oracle():
    with IO.installed():
        yield


def _utd_of(B):
    return 2 if B % 2 == 0 else next((u for u in range(3, B + 1) if B % u == 0), 1)


def _core_of(run, fuse):
    """a fresh agent holding the parameters the case's oracle run started from"""
    cfg = run["cfg"]
    trunk, theta = IO.init_params(cfg, run["seed"])
    return AH.load_leaves(IO.make_core(cfg, run["B"], fuse=fuse), cfg, trunk, theta)


def _leaf_checks(core, cfg):
    E = 256 * cfg.n_cam
    assert core.use_proprio is False and int(core.L.serl_agent_use_proprio(core._h)) == 0
    assert not any(k.startswith("enc/proprio") for k in core.leaves)
    w1c, w1a = core.leaves["critic/w1"], core.leaves["actor/w1"]
    assert w1c == cfg.ensemble * (E + cfg.A) * (cfg.critic_dims or (cfg.hidden,))[0] if getattr(cfg, "critic_dims", None) else w1c == cfg.ensemble * (E + cfg.A) * cfg.hidden
    assert w1a == E * ((cfg.policy_dims[0]) if getattr(cfg, "policy_dims", None) else cfg.hidden)


# ---- oracle parity -----------------------------------------------------------------------------------------------------------
@FUSE
@pytest.mark.parametrize("name", IO.IDS)
def test_update_critics_matches_the_oracle(gpu, name, fuse):
    run = IO.oracle_run(name, "critics")
    cfg, B, st, aux = run["cfg"], run["B"], run["state"], run["aux"]
    core = _core_of(run, fuse)
    _leaf_checks(core, cfg)
    core.update_critics(AH.batch_to_device(cfg, run["batch"]), AH.noise_to_device(cfg, run["noise"]))
    fig = _Figures(f"update_critics {name} {'fused' if fuse else 'unfused'}")
    _info(fig, core.read_info(), run["info"], ("critic_loss", "predicted_qs", "target_qs"))
    fig.add("q", AH.rel_err(core.debug("q", cfg.ensemble * B).reshape(cfg.ensemble, B), aux["q"].numpy()))
    fig.add("target_q", AH.rel_err(core.debug("target_q", B), aux["target_q"].numpy()))
    fig.add("next logp", AH.rel_err(core.debug("logp", B), aux["next_logp"].numpy()))
    MR.grads(fig, cfg, core, aux["grads"], "g_critic")
    fig.check()
    _compare_state(cfg, st, core)
    assert core.step == st.step == 1
    assert core.debug("ctr_nonzero", 1)[0] == 0


@FUSE
@pytest.mark.parametrize("name", IO.IDS)
def test_update_high_utd_matches_the_oracle(gpu, name, fuse):
    utd = _utd_of(IO.CASES[name]["rows"])
    run = IO.oracle_run(name, ("high_utd", utd))
    cfg, B, st = run["cfg"], run["B"], run["state"]
    core = _core_of(run, fuse)
    core.update_high_utd(AH.batch_to_device(cfg, run["batch"]), utd, AH.noise_to_device(cfg, run["noise"]))
    fig = _Figures(f"update_high_utd({utd}) {name} {'fused' if fuse else 'unfused'}")
    _info(fig, core.read_info(), run["info"], ("critic_loss", "predicted_qs", "target_qs", "actor_loss", "temperature", "entropy", "temperature_loss"))
    MR.grads(fig, cfg, core, run["aux"]["g_actor"], "g_actor")
    fig.check()
    _compare_state(cfg, st, core, steps=utd + 1)
    assert core.step == st.step == utd + 1
    assert core.debug("ctr_nonzero", 1)[0] == 0


@FUSE
@pytest.mark.parametrize("kind,utd", [("critics", 1), ("high_utd", 5)], ids=["critics", "high_utd5"])
def test_frame_stack_of_two_matches_the_oracle(gpu, kind, utd, fuse):
    """case 4: SmallEncoder, num_stack 2, two cameras 47x33, 65 rows, A = 4 -- the oracle's image-only agent with conv0 widened to
    six channels, fed channel-folded frames (tests/stacked_oracle.py); one update_critics, and one update_high_utd(5), each from
    the initial state.  The batch seed is image_only.STACK_SEED, chosen on the CPU for ADAM_MARGIN (tests/test_image_only_cpu.py)"""
    cfg, wcfg, T, B, st, core = IO.stack_pair(fuse)
    assert core.leaves["enc/0/conv0/kernel"] == 9 * 3 * T * 32 and not any(k.startswith("enc/proprio") for k in core.leaves)
    pb, noise, fr = IO.stack_batch(cfg, wcfg, T, B, utd)
    ob, db = SO.oracle_batch(wcfg, T, pb, fr), SO.device_batch(wcfg, T, pb, fr)
    if kind == "critics":
        info, _ = O.update_critics(st, ob, O.noise_to_torch(noise, torch.float64))
        core.update_critics(db, AH.noise_to_device(cfg, noise))
        names = ("critic_loss", "predicted_qs", "target_qs")
    else:
        info, _ = O.update_high_utd(st, ob, O.noise_to_torch(noise, torch.float64), utd)
        core.update_high_utd(db, utd, AH.noise_to_device(cfg, noise))
        names = ("critic_loss", "predicted_qs", "target_qs", "actor_loss", "temperature", "entropy", "temperature_loss")
    fig = _Figures(f"stack2 {kind} {'fused' if fuse else 'unfused'}")
    _info(fig, core.read_info(), info, names)
    fig.check()
    steps = 1 if kind == "critics" else utd + 1
    _compare_state(cfg, st, core, steps=steps)
    assert core.step == st.step == steps


# ---- the rider -----------------------------------------------------------------------------------------------------------------
@FUSE
def test_the_actions_ride_into_the_critic_input(gpu, fuse):
    """after the critic forward of case 2 the online critic's input (tap "x": where the rider writes; the target critic takes the
    policy's next actions) has the batch's actions in columns [E, E + A) bit for bit, and the camera codes in columns [0, E) (the
    oracle's code of that pass, at TOL: the library has no tap of its own for it)"""
    run = IO.oracle_run("c2_frozen_2cam_33x47_B65_A5_E10", "critics")
    cfg, B = run["cfg"], run["B"]
    core = _core_of(run, fuse)
    core.update_critics(AH.batch_to_device(cfg, run["batch"]), AH.noise_to_device(cfg, run["noise"]))
    E, A = 256 * cfg.n_cam, cfg.A
    x = core.debug("x", B * (E + A)).reshape(B, E + A)
    assert _bits_equal(x[:, E:], run["batch"]["action"])
    assert AH.rel_err(x[:, :E], run["aux"]["enc_obs"].numpy()) < TOL and run["aux"]["enc_obs"].shape == (B, E)


# ---- the state is never read ---------------------------------------------------------------------------------------------------
def test_the_state_is_never_read(gpu):
    name = "c1_frozen_1cam_B6_A3"
    cfg, B = IO.case_config(name)
    got = []
    for fill in (0.0, float("nan")):
        _, core = IO.make_pair(cfg, B)
        for it in range(2):
            b = AH.synth_batch(cfg, B, seed=50 + it)
            b["state"][:] = fill
            b["next_state"][:] = fill
            db = AH.batch_to_device(cfg, b)
            noise = AH.noise_to_device(cfg, O.make_noise(cfg, B, seed=60 + it, utd_ratio=1))
            core.update_critics(db, noise) if it == 0 else core.update_high_utd(db, 1, noise)
        state = torch.full((B, cfg.S), fill, device="cuda")
        act = torch.tensor(b["action"], device="cuda")
        frames = db.frames[0].contiguous()
        outs = [core.sample_actions(frames, state, None).cpu().numpy(), core.eval_q(frames, state, act).cpu().numpy(),
                core.eval_q(frames, state, act, target=True).cpu().numpy()]
        outs += [v.cpu().numpy() for v in core.eval_policy(frames, state, act).values()]
        assert all(np.isfinite(o).all() for o in outs)
        got.append((IO.all_bits(core), core.read_info(), outs))
    (b0, i0, o0), (b1, i1, o1) = got
    assert i0 == i1 and all(np.isfinite(v) for v in i1.values())
    for key in b0:
        assert _bits_equal(b0[key], b1[key]), key
    for a, b in zip(o0, o1):
        assert _bits_equal(a, b)


def test_a_null_state_pointer_is_accepted(gpu):
    """serl_batch.state and dev_state NULL: the update and sample_actions run and give the bits of the run with a state tensor"""
    cfg, B = IO.case_config("c1_frozen_1cam_B6_A3")
    res = []
    for null in (False, True):
        _, core = IO.make_pair(cfg, B)
        db = AH.batch_to_device(cfg, AH.synth_batch(cfg, B, seed=51))
        if null:
            db.cstruct.state = None
        core.update_high_utd(db, 1, AH.noise_to_device(cfg, O.make_noise(cfg, B, seed=61, utd_ratio=1)))
        out = torch.empty((B, cfg.A), dtype=torch.float32, device="cuda")
        st = None if null else C.c_void_p(db.state[0].data_ptr())
        rc = core.L.serl_agent_sample_actions(core._h, C.c_void_p(db.frames[0].contiguous().data_ptr()), st, B, None, C.c_void_p(out.data_ptr()), core._stream())
        assert rc == 0
        res.append((IO.all_bits(core), out.cpu().numpy()))
    for key in res[0][0]:
        assert _bits_equal(res[0][0][key], res[1][0][key]), key
    assert _bits_equal(res[0][1], res[1][1])


# ---- the default agent is untouched; launch counts ------------------------------------------------------------------------------
def _run_pair(core, cfg, B, seed):
    db = AH.batch_to_device(cfg, AH.synth_batch(cfg, B, seed=seed))
    dn = AH.noise_to_device(cfg, O.make_noise(cfg, B, seed=seed + 100, utd_ratio=2))
    torch.cuda.synchronize()
    l0 = _launches()
    core.update_critics(db, dn)
    core.update_high_utd(db, 2, dn)
    torch.cuda.synchronize()
    return _launches() - l0


@pytest.mark.parametrize("encoder_type", ["resnet-pretrained", "small"])
def test_the_switch_with_use_proprio_true_is_the_agent_without_it(gpu, encoder_type):
    kw = dict(B=6, encoder_type=encoder_type, seed=3)
    with_switch = IO.drq_agent(use_proprio=True, **kw)
    without = IO.drq_agent(use_proprio=True, image_only=False, **kw)
    assert list(with_switch.core.leaves.items()) == list(without.core.leaves.items()) and with_switch.config == without.config
    assert "enc/proprio/dense/kernel" in without.core.leaves and "use_proprio" not in without.config
    cfg = O.Config(image_keys=("wrist",), H=32, W=32, S=5, A=3, encoder_type=encoder_type)
    n = [_run_pair(a.core, cfg, 6, 300) for a in (with_switch, without)]
    assert n[0] == n[1], n
    assert with_switch.core.read_info() == without.core.read_info()
    want = IO.all_bits(without.core)
    for key, v in IO.all_bits(with_switch.core).items():
        assert _bits_equal(v, want[key]), key


def _utd1_launches(core, cfg, B, seed):
    db = AH.batch_to_device(cfg, AH.synth_batch(cfg, B, seed=seed))
    dn = AH.noise_to_device(cfg, O.make_noise(cfg, B, seed=seed + 100, utd_ratio=1))
    torch.cuda.synchronize()
    l0 = _launches()
    core.update_high_utd(db, 1, dn)
    torch.cuda.synchronize()
    return _launches() - l0


@FUSE
@pytest.mark.parametrize("name", ["c1_frozen_1cam_B6_A3", "c3_small_1cam_B6_A3_adamw_clip"])
def test_an_image_only_update_launches_no_more_kernels_than_its_proprio_twin(gpu, name, fuse):
    n = {}
    for flag in (False, True):
        cfg, B = IO.case_config(name, use_proprio=flag)
        n[flag] = _utd1_launches(IO.make_pair(cfg, B, fuse=fuse)[1], cfg, B, 310)
    print(f"{name} {'fused' if fuse else 'unfused'}: chain launches per update_high_utd(1): image-only {n[False]}, proprio {n[True]}")
    assert n[False] <= n[True], n


# ---- cross-check without the oracle ---------------------------------------------------------------------------------------------
def test_image_only_equals_a_proprio_agent_with_zero_proprio_rows(gpu):
    cfg_p, B = IO.case_config("c1_frozen_1cam_B6_A3", use_proprio=True)
    cfg_i, _ = IO.case_config("c1_frozen_1cam_B6_A3")
    B = 7
    trunk, theta = IO.init_params(cfg_p, 11)
    E = 256
    theta = dict(theta)
    theta["critic/w1"] = theta["critic/w1"].copy()
    theta["actor/w1"] = theta["actor/w1"].copy()
    theta["critic/w1"][:, E:E + 64, :] = 0
    theta["actor/w1"][E:E + 64, :] = 0
    prop = AH.load_leaves(IO.make_core(cfg_p, B), cfg_p, trunk, theta)
    th_i = {k: v for k, v in theta.items() if not k.startswith("enc/proprio")}
    th_i["critic/w1"] = np.ascontiguousarray(np.delete(theta["critic/w1"], np.s_[E:E + 64], axis=1))
    th_i["actor/w1"] = np.ascontiguousarray(theta["actor/w1"][:E])
    img = AH.load_leaves(IO.make_core(cfg_i, B), cfg_i, trunk, th_i)
    b = AH.synth_batch(cfg_p, B, seed=9)
    frames = torch.tensor(b["obs"]["wrist"], device="cuda")[None].contiguous()
    state, act = torch.tensor(b["state"], device="cuda"), torch.tensor(b["action"] * 0.9, device="cuda")
    fig = _Figures("image-only against zeroed proprio rows")
    for target in (False, True):
        fig.add(f"q target={target}", AH.rel_err(img.eval_q(frames, state, act, target=target).cpu().numpy(),
                                                 prop.eval_q(frames, state, act, target=target).cpu().numpy()))
    pi, pp = img.eval_policy(frames, state, act), prop.eval_policy(frames, state, act)
    for k in pp:
        fig.add(k, AH.rel_err(pi[k].cpu().numpy(), pp[k].cpu().numpy()))
    fig.add("argmax action", AH.rel_err(img.sample_actions(frames, state, None).cpu().numpy(), prop.sample_actions(frames, state, None).cpu().numpy()))
    fig.check()


# ---- read-only calls -------------------------------------------------------------------------------------------------------------
def test_eval_losses_equals_the_updates_own_info_and_changes_nothing(gpu):
    cfg, B = IO.case_config("c1_frozen_1cam_B6_A3")
    _, core = IO.make_pair(cfg, B)
    db = AH.batch_to_device(cfg, AH.synth_batch(cfg, B, seed=11))
    noise = O.make_noise(cfg, B, seed=12)
    before = IO.all_bits(core)
    dry = core.eval_losses(db, AH.noise_to_device(cfg, noise))
    torch.cuda.synchronize()
    for key, v in IO.all_bits(core).items():
        assert _bits_equal(v, before[key]), key
    core.update(db, noise=AH.noise_to_device(cfg, noise))
    for k, v in core.read_info().items():
        assert dry[k] == v, (k, dry[k], v)


def test_read_only_calls_leave_the_agent_byte_for_byte(gpu):
    keys, H, W, S, A, B = ("wrist",), 32, 32, 5, 3, 6
    agent = IO.drq_agent(keys, H, W, S, A, B, seed=7)
    assert agent.config["use_proprio"] is False and agent.core.use_proprio is False
    agent.update_high_utd(IO.flat_batch(keys, H, W, S, A, B, 10), utd_ratio=2)
    torch.cuda.synchronize()
    before = _state_of(agent)
    batch = IO.flat_batch(keys, H, W, S, A, B, 11, state=float("nan"))
    obs = {k: (v[:, 0] if k != "state" else v[:, None]).cpu().numpy() for k, v in batch["observations"].items()}      # state (n, T = 1, S)
    act = batch["actions"].cpu().numpy()
    q, qt = agent.q_values(obs, act), agent.q_values(obs, act, target=True)
    stats = agent.policy_stats(obs, act)
    assert q.shape == qt.shape == (10, B) and np.isfinite(q).all() and np.isfinite(qt).all() and np.isfinite(stats["log_prob"]).all()
    assert np.array_equal(stats["mode"], agent.sample_actions(obs, argmax=True))
    ev = agent.evaluate_batch(batch, side="next_observations")
    losses = agent.evaluate_losses(batch)
    assert np.isfinite(ev["q"]).all() and losses is not None
    torch.cuda.synchronize()
    assert _same(before, _state_of(agent)) == []


# ---- checkpoints, export, snapshots ----------------------------------------------------------------------------------------------
def test_checkpoint_roundtrip_export_snapshot_and_the_refusals_across_proprio(gpu):
    from serl_amd.utils.checkpoint import load_state_dict
    keys, H, W, S, A, B = ("wrist",), 32, 32, 5, 3, 6
    agent = IO.drq_agent(keys, H, W, S, A, B, seed=7, critic_ensemble_size=2, critic_subsample_size=None)
    for i in range(2):
        agent.update_high_utd(IO.flat_batch(keys, H, W, S, A, B, 10 + i), utd_ratio=2)
    tree = agent.state.params
    for mod in ("modules_actor", "modules_critic"):
        enc = tree.get(mod, {}).get("encoder", {})
        assert "Dense_0" not in enc and "LayerNorm_0" not in enc
    assert sorted(tree["modules_actor"]["encoder"]) == ["encoder_wrist"]
    assert tree["modules_actor"]["network"]["Dense_0"]["kernel"].shape == (256, 256)
    assert tree["modules_critic"]["network"]["Dense_0"]["kernel"].shape == (2, 256 + A, 256)
    # get(set(x)) == x on every leaf
    for leaf, n in agent.core.leaves.items():
        if leaf.startswith("trunk/"):
            continue
        v = np.random.default_rng(n).standard_normal(n).astype(np.float32)
        old = agent.core.get("target_params", leaf)
        agent.core.set("target_params", leaf, v)
        assert _bits_equal(agent.core.get("target_params", leaf), v), leaf
        agent.core.set("target_params", leaf, old)
    # a snapshot equals serl_agent_get leaf by leaf
    snap = agent.snapshot(("params", "target_params", "opt_states"))
    sd = {"params": snap.params, "target_params": snap.target_params, "opt_states": snap.opt_states, "step": snap.step}
    live = {"params": agent.state.params, "target_params": agent.state.target_params}

    def flat(t, pre=()):
        for k in sorted(t):
            yield from (flat(t[k], pre + (k,)) if isinstance(t[k], dict) else [(pre + (k,), np.asarray(t[k]))])
    for sec in live:
        a, b = dict(flat(sd[sec])), dict(flat(live[sec]))
        assert set(a) == set(b)
        for p in a:
            assert np.array_equal(a[p], b[p]), (sec, p)
    # round trip, byte for byte, and an identical next update
    fresh = IO.drq_agent(keys, H, W, S, A, B, seed=1, critic_ensemble_size=2, critic_subsample_size=None)
    load_state_dict(fresh, sd)
    fresh._rng_key = agent._rng_key.copy()
    want = IO.all_bits(agent.core)
    for key, v in IO.all_bits(fresh.core).items():
        assert _bits_equal(v, want[key]), key
    nxt = IO.flat_batch(keys, H, W, S, A, B, 20)
    agent.update_high_utd(nxt, utd_ratio=1)
    fresh.update_high_utd(nxt, utd_ratio=1)
    want = IO.all_bits(agent.core)
    for key, v in IO.all_bits(fresh.core).items():
        assert _bits_equal(v, want[key]), ("after the next update", key)
    # refused whole, both ways
    prop = IO.drq_agent(keys, H, W, S, A, B, seed=3, use_proprio=True, critic_ensemble_size=2, critic_subsample_size=None)
    for src, dst, pat in ((agent, prop, r"the state holds no proprio branch .*this agent has one \(use_proprio=True\); nothing was loaded"),
                          (prop, agent, r"the state holds the proprio branch .*this agent is image-only \(use_proprio=False\).*nothing was loaded")):
        before, step_before = IO.all_bits(dst.core), dst.state.step
        state = {"params": src.state.params, "target_params": src.state.target_params, "opt_states": src.state.opt_states, "step": 5}
        with pytest.raises(ValueError, match=pat):
            load_state_dict(dst, state)
        assert dst.state.step == step_before
        for key, v in IO.all_bits(dst.core).items():
            assert _bits_equal(v, before[key]), ("touched by the refused restore", key)


# ---- two shards -------------------------------------------------------------------------------------------------------------------
def _rows(d, lo, hi):
    """rows [lo, hi) of a synth batch or of a noise dict (redq_idx is per update, not per row)"""
    return {k: (v if k == "redq_idx" else {c: m[lo:hi] for c, m in v.items()} if isinstance(v, dict) else v[lo:hi]) for k, v in d.items()}


def test_two_shards_sum_to_the_full_batch(gpu):
    """tests/test_policy_fixed_gpu.py::test_two_shards_of_a_batch_equal_the_full_batch on case 2, as shards of 32 and 33 rows through
    set_shard and the phase API: two ranks' gradient and scalar sums are the full batch's, at that test's bound (float32 sums
    re-associated)"""
    run0 = IO.oracle_run("c2_frozen_2cam_33x47_B65_A5_E10", "critics")
    cfg, B = run0["cfg"], run0["B"]
    trunk, theta = IO.init_params(cfg, run0["seed"])
    b, noise = run0["batch"], O.make_noise(cfg, B, seed=9, utd_ratio=1)

    def run(lo, rows, sharded):
        core = AH.load_leaves(IO.make_core(cfg, rows, agent_seed=7), cfg, trunk, theta)
        if sharded:
            core.set_shard(lo, B)
        db, dn = AH.batch_to_device(cfg, _rows(b, lo, lo + rows)), AH.noise_to_device(cfg, _rows(noise, lo, lo + rows))
        core.begin_update()
        core.encode(db)
        core.critic_grads(0, rows, B, dn)
        (clo, chi), (alo, ahi) = MR.tap_ranges(core)["g_critic"], MR.tap_ranges(core)["g_actor"]
        gc, sc = core.debug("g_critic", chi - clo).astype(np.float64), core.debug("scalars", 3).astype(np.float64)
        core.actor_grads(B, dn)
        return gc, sc, core.debug("g_actor", ahi - alo).astype(np.float64), core.debug("scalars", 6)[3:6].astype(np.float64)
    full = run(0, B, False)
    parts = [run(0, 32, True), run(32, 33, True)]
    for i, what in enumerate(("g_critic", "critic scalars", "g_actor", "actor scalars")):
        err = AH.rel_err(parts[0][i] + parts[1][i], full[i])
        print(f"two shards (32 + 33 rows) vs the full batch, {what}: {err:.2e}")
        assert np.abs(full[i]).max() > 0 and err < 1e-5, what


# ---- reward labels -----------------------------------------------------------------------------------------------------------------
def test_reward_labels_equal_those_of_the_proprio_twin(gpu):
    from serl_amd.networks.reward_classifier import Classifier
    keys, H, W, S, A, B = ("wrist",), 32, 32, 5, 3, 6
    labels = []
    for flag in (False, True):
        agent = IO.drq_agent(keys, H, W, S, A, B, seed=7, use_proprio=flag)
        p = CO.make_params(keys, H, W, 11)
        clf = Classifier(keys, H, W, max_batch=B).load_flat({k: v for k, v in p.items() if not k.startswith("trunk/")})
        for leaf in (k for k in p if k.startswith("trunk/")):      # the agent's own trunk: labels from the update's features
            clf.set(leaf, agent.core.get("params", leaf))
        agent.set_reward_classifier(clf)
        agent.update_critics(IO.flat_batch(keys, H, W, S, A, B, 10))
        labels.append(agent.last_reward_labels())
    assert _bits_equal(labels[0][0], labels[1][0]) and _bits_equal(labels[0][1], labels[1][1])


# ---- the reference's own code: tests/golden/imgonly_*.npz ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", IO.UPDATE_GOLDEN)
def test_hip_update_matches_the_reference_golden(gpu, name):
    """tests/test_golden_update_gpu.py::test_hip_update_matches_the_reference_golden on imgonly_update_<name>.npz (injected noise):
    the reference's own create_drq(use_proprio=False) and update code"""
    import golden_replay as GR
    g = IO.load_golden(name)
    cfg = g["cfg"]
    agent = IO.reference_agent(cfg, g["B"])
    assert agent.core.use_proprio is False and not any(k.startswith("enc/proprio") for k in agent.core.leaves)
    AH.load_leaves(agent.core, cfg, *O.init_params(cfg, g["meta"]["param_seed"]))
    GR.replay(agent, g, label=f"imgonly_update_{name}")
    assert agent.core.debug("ctr_nonzero", 1)[0] == 0


def test_reference_init_then_one_update_matches_the_reference(gpu):
    """tests/test_init_reference_gpu.py::test_reference_init_then_one_update_matches_the_reference on imgonly_init_drq.npz: from the
    seed only, param_init="reference", the tree without the proprio branch"""
    import golden_replay as GR
    import init_golden_helpers as IG
    from oracle import golden_update as G
    from serl_amd.utils import init as pinit
    npz, cfg, recs, _ = IO.init_golden()
    g = G.unpack(npz)
    g["cfg"] = cfg
    agent = IO.reference_agent(cfg, g["B"], param_init="reference")
    core = agent.core
    assert core.use_proprio is False and set(recs) == {k for k in core.leaves if not k.startswith("trunk/")}
    bad = [m for n in sorted(recs) for sec in ("params", "target_params") for m in [IG.mismatch(n, recs[n], core.get(sec, n))] if m]
    assert not bad, bad
    for n in recs:
        for tx in ("critic", "actor", "temperature"):
            assert not core.get(f"opt/{tx}/mu", n).any() and not core.get(f"opt/{tx}/nu", n).any()
    assert [int(v) for v in agent.state.rng] == g["meta"]["rng0"] == [int(v) for v in npz["init_rng"]]
    assert np.array_equal(core.get("params", "trunk/conv_init"), pinit.init_trunk(0)["trunk/conv_init"].reshape(-1))
    assert [s["kind"] for s in g["steps"]] == ["high_utd"]
    GR.replay(agent, g, seed_only=True, label="imgonly_init_drq")
