"""GPU: action widths above 64 (serl_agent_opts.wide_actions, wide_actions=True) -- the wide head rows of serl_amd/csrc/head_wide.h
under the whole update chain and the read-only calls, against the fp64 oracle, on the case table of tests/wide_actions.py.
TOL = 1e-4 as in tests/test_mlp_widths_gpu.py; log pi of given actions at max(1e-4, 4 x the fp32 restatement's deviation), the
bound of tests/test_evaluate_gpu.py.  Without the switch every A > 64 case fails when its agent is made ("bad dims")."""
import numpy as np
import pytest
import torch

import agent_helpers as AH
import eval_oracle as EO
import mlp_widths as MW
import test_evaluate_gpu as TE
import wide_actions as WA
from test_agent_gpu import _compare_state
from test_chain_fusion_gpu import _assert_state_bits, _bits_equal, _launches
from test_mlp_widths_gpu import _Figures, _info
from test_sample_best_gpu import _check as _check_best, _reference as _best_reference

pytestmark = pytest.mark.gpu
INFO = ("critic_loss", "predicted_qs", "target_qs", "actor_loss", "temperature", "entropy", "temperature_loss")


@pytest.mark.parametrize("name", list(WA.CASES))
def test_a_full_update_matches_the_oracle_in_both_schedules(gpu, name):
    """critic, actor, temperature, Adam and EMA: fused == un-fused bit for bit; info scalars (entropy = -mean log pi over A columns),
    every actor-side gradient leaf and the state after the step against the fp64 oracle"""
    run = WA.oracle_run(name)
    with WA.oracle_of(run["cfg"]):
        _check_update(name, run)


def _check_update(name, run):
    cfg, B = run["cfg"], run["B"]
    cores = [WA.make_core(cfg, B, run["leaves"], fuse=f) for f in (True, False)]
    for core in cores:
        core.update_high_utd(AH.batch_to_device(cfg, run["batch"]), 1, AH.noise_to_device(cfg, run["noise"]))
    core = cores[0]
    assert core.read_info() == cores[1].read_info() and _bits_equal(core.debug("logp", B), cores[1].debug("logp", B)), name
    _assert_state_bits(cfg, core, cores[1], name)
    fig = _Figures(name)
    _info(fig, core.read_info(), run["info"], INFO)
    sl, _ = AH.leaf_slices(cfg)      # the actor optimizer's gradient: from the proprio branch (pixels) or the policy's first layer to its last head leaf
    lo0 = sl.get("enc/proprio/dense/kernel", sl["actor/w1"])[0]
    g = core.debug("g_actor", max(hi for k, (_, hi) in sl.items() if k.startswith("actor/")) - lo0)
    for k, gv in run["g_actor"].items():
        fig.add(f"g_actor {k}", AH.rel_err(g[sl[k][0] - lo0:sl[k][1] - lo0], gv.numpy().reshape(-1)))
    # log pi of the actor loss, a sum over A columns, per row: four times the float32 oracle's own deviation where that is above TOL
    # (the fixed std's pinned oracle runs in float64 alone: TOL itself)
    dev32 = 0.0 if "fixed" in name else EO.row_error(WA.oracle_run(name, torch.float32)["logp"], run["logp"])
    print(f"{name}: log pi float32 oracle deviation {dev32:.2e}")
    fig.add("log pi", EO.row_error(core.debug("logp", B), run["logp"]), max(TE.TOL, 4.0 * dev32))
    fig.check()
    _compare_state(cfg, run["state"], core, steps=2)
    assert core.step == run["state"].step == 2 and core.debug("ctr_nonzero", 1)[0] == 0


def _inputs(cfg, n, N, unit_row=None):
    rng = np.random.default_rng(11)
    state, eps = rng.standard_normal((n, cfg.S)).astype(np.float32), rng.standard_normal((N, n, cfg.A)).astype(np.float32)
    actions = EO.scaled_actions(rng.uniform(-1, 1, (n, cfg.A)))
    if unit_row is not None:
        actions[unit_row, cfg.A - 1] = 1.0      # exactly 1.0 in the last, ragged block: no finite pre-image
    return state, eps, actions


@pytest.mark.parametrize("std,squash,regime", [("exp", True, "init"), ("uniform", False, "init"), ("softplus", True, "trained")])
def test_read_only_calls_at_200_columns_match_the_restatement_and_leave_the_state_alone(gpu, std, squash, regime):
    cfg = WA.config(200, std, squash)
    lv = TE._leaves(cfg, regime)
    core = WA.make_core(cfg, 72, lv)
    n, N = 6, 4
    state, eps, actions = _inputs(cfg, n, N)
    before = {k: core.get(sec, k).copy() for sec in ("params", "target_params") for k in core.leaves}
    r64, err32 = EO.log_prob_yardstick(cfg, *lv, {}, state, actions)
    TE._check(f"A200 {std} {squash} {regime}", TE._core_eval(core, None, TE._dev(state), TE._dev(actions)), r64, err32)
    ref = _best_reference(cfg, lv, {}, state, eps, "min")
    _check_best(f"A200 best {std}", core, None, state, eps, ref, "min")                                    # sample_actions(num_candidates=4)
    q = core.eval_q(None, TE._dev(state), TE._dev(ref["actions"].astype(np.float32))).cpu().numpy()           # q_values with [n, N, A]
    assert q.shape == (cfg.ensemble, n, N) and np.abs(q - ref["q"]).max() < TE.TOL
    if squash:      # a component of exactly 1.0: the row's log-density is not finite, as the reference's is; the other rows are
        state1, _, act1 = _inputs(cfg, n, N, unit_row=2)
        lp = core.eval_policy(None, TE._dev(state1), TE._dev(act1))["log_prob"].cpu().numpy()
        assert not np.isfinite(lp[2]) and np.isfinite(np.delete(lp, 2)).all(), lp
    after = {k: core.get(sec, k) for sec in ("params", "target_params") for k in core.leaves}
    assert all(_bits_equal(before[k], after[k]) for k in before) and core.debug("ctr_nonzero", 1)[0] == 0


@pytest.mark.parametrize("A", [65, 200, 256])
def test_a_rows_head_outputs_do_not_depend_on_the_row_count(gpu, A):
    """row 0 from a launch of 1 row and from a launch of 65 rows: sample, distribution and log pi bit for bit"""
    cfg = WA.config(A)
    core = WA.make_core(cfg, 72, TE._leaves(cfg, "init"))
    state, eps, actions = _inputs(cfg, 65, 1)
    outs = []
    for n in (1, 65):
        s, e, a = TE._dev(state[:n]), TE._dev(eps[0, :n]), TE._dev(actions[:n])
        pol = core.eval_policy(None, s, a)
        outs.append([core.sample_actions(None, s, e)[0], core.sample_actions(None, s, None)[0]] + [pol[k][0] for k in ("mean", "std", "log_prob")])
    assert all(_bits_equal(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(*outs))


@pytest.mark.parametrize("A", [7, 64])
def test_the_switch_is_inert_up_to_64_columns(gpu, A):
    """params, target, optimizer state and info after two updates, and the launch count, of the agent with and without the switch"""
    cfg = WA.config(A)
    lv, n = TE._leaves(cfg, "init"), []
    on, off = (WA.make_core(cfg, 9, lv, wide_actions=w) for w in (True, False))
    assert on.spec.to_c().wide_actions == 1 and off.spec.to_c().wide_actions == 0
    for core in (on, off):
        torch.cuda.synchronize()
        l0 = _launches()
        for it in range(2):
            core.update_high_utd(AH.batch_to_device(cfg, AH.synth_batch(cfg, 9, seed=300 + it)), 1)
        torch.cuda.synchronize()
        n.append(_launches() - l0)
    assert on.read_info() == off.read_info() and n[0] == n[1], n
    _assert_state_bits(cfg, on, off, f"A{A}")


def test_checkpoint_roundtrip_and_another_act_dim_at_200_columns(gpu, tmp_path):
    from serl_amd.agents.flax_tree import net_spec_of
    from serl_amd.utils.checkpoint import restore_checkpoint, save_checkpoint
    from test_mlp_widths_gpu import _all_bits, _flat_batch

    def agent(A, seed):
        return MW.sac_agent(64, seed=seed, B=8, S=10, A=A, critic_ensemble_size=2, wide_actions=True)
    a, b, other = agent(200, 7), agent(200, 2), agent(199, 2)
    assert a.core.spec.wide_actions and net_spec_of(a.core).wide_actions and not net_spec_of(agent(64, 1).core).wide_actions
    a.update_high_utd(_flat_batch(10, 200, 8, 10), utd_ratio=2)
    save_checkpoint(str(tmp_path / "wide"), a, step=a.state.step)
    restore_checkpoint(str(tmp_path / "wide"), b, restore_rng=True)
    for x in (a, b):
        x.update_high_utd(_flat_batch(10, 200, 8, 20), utd_ratio=1)
    want = _all_bits(a)
    assert all(_bits_equal(v, want[k]) for k, v in _all_bits(b).items())
    with pytest.raises(ValueError, match=r"leaf '[a-z0-9/]+' has \d+ elements in this agent, the state holds \d+"):
        restore_checkpoint(str(tmp_path / "wide"), other)


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "unfused"])
def test_two_shards_draw_and_sum_to_the_full_batch_at_200_columns(gpu, fuse):
    """tests/test_agent_gpu.py::test_device_noise_is_indexed_by_the_global_sample with the actor phase, at its bound: production noise
    (the head rows draw eps at the global row; un-fused, gen_noise does), every rank a fresh agent of the same seed under set_shard"""
    cfg, B = WA.config(200, backup_entropy=True), 16
    lv, b, redq = TE._leaves(cfg, "init"), AH.synth_batch(cfg, B, seed=5), {"redq_idx": np.array([[0, 1]], np.int32)}
    sl, _ = AH.leaf_slices(cfg)
    pc, pa0, pa1 = sl["critic/head/bias"][1], sl["actor/w1"][0], sl["actor/logstd/bias"][1]

    def run(parts):
        out, per = None, B // parts
        for r in range(parts):
            core = WA.make_core(cfg, per, lv, fuse=fuse, agent_seed=7)
            core.set_shard(r * per, B if parts > 1 else 0)
            core.begin_update()
            core.encode(AH.batch_to_device(cfg, {k: v[r * per:(r + 1) * per] if not isinstance(v, dict) else v for k, v in b.items()}))
            core.critic_grads(0, per, B, redq)
            got = [core.debug("g_critic", pc), core.debug("scalars", 3)]
            core.actor_grads(B, None)
            got += [core.debug("g_actor", pa1 - pa0), core.debug("scalars", 6)[3:6]]
            out = [x.astype(np.float64) + (0 if out is None else out[i]) for i, x in enumerate(got)]
        return out
    full, halves = run(1), run(2)
    for what, f, h in zip(("g_critic", "critic scalars", "g_actor", "actor scalars"), full, halves):
        print(f"two shards vs the full batch, {what}: {AH.rel_err(h, f):.2e}")
        assert np.abs(f).max() > 0 and AH.rel_err(h, f) < 1e-5, what


def test_bc_update_and_argmax_inference_at_200_columns_match_the_statement(gpu):
    """tests/test_image_only_bc_gpu.py's comparison on one camera, B = 65, A = 200 (serl_bc_create_wide)"""
    import bc_oracle as BO
    import image_only_bc as IB
    import learner_regimes as LR
    from serl_amd import jaxrng as J
    from serl_amd.agents.bc import BCAgent
    from test_bc_gpu import _close
    from test_learner_regimes_gpu import _check_bc_step
    with IB.installed():
        r64, r32 = IB.run(WA.BC_CASE, steps=1), IB.run(WA.BC_CASE, torch.float32, steps=1)
        cfg, B, s64 = r64["cfg"], r64["B"], r64["steps"][0]
        agent = BCAgent(cfg.image_keys, cfg.H, cfg.W, cfg.S, cfg.A, seed_key=J.prngkey(0), max_batch=B, use_proprio=False, wide_actions=True)
        agent.load_flat(r64["trunk"]).load_flat(r64["theta"])
        inp = s64["inp"]
        _, info = agent.update(LR.bc_batch(inp["frames"], inp["state"], inp["action"]), masks=inp["masks"])
        _check_bc_step("bc A200", cfg, agent, dict(info), s64, r32["steps"][0])
        inf = IB.inputs(cfg, B, 90)
        obs = {**{k: torch.tensor(v[:, None], device="cuda") for k, v in inf["frames"].items()}, "state": torch.tensor(inf["state"], device="cuda")}
        _close(agent.sample_actions(obs, argmax=True), BO.sample_actions(r64["state"], BO.features(r64["trunk"], cfg, inf["frames"]), inf["state"]).numpy())
        with pytest.raises(Exception, match="act_dim 65 unsupported"):      # without the switch: refused as always
            BCAgent(cfg.image_keys, cfg.H, cfg.W, cfg.S, 65, seed_key=J.prngkey(0), max_batch=B, use_proprio=False)
