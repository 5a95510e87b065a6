"""GPU: Q for N candidate actions per observation in one pass -- q_values / AgentCore.eval_q with actions [n, N, A] over
serl_agent_eval_q_actions and critic_fanout_kernel (heads.hip), the reference's multiple_action_q_function.  Without the feature
every test fails: the symbol is missing.  Reference: tests/eval_oracle.py::evaluate in fp64, once per candidate column, stacked on the
last axis; bound: the TOL of tests/test_evaluate_gpu.py under agent_helpers.rel_err.  Measured worst on an MI355X: 6.0e-7 (c4)."""
import numpy as np
import pytest
import torch

import agent_helpers as AH
import eval_oracle as EO
import mlp_plain as MP
import mlp_ragged as MR
import policy_fixed as PF
import stacked_oracle as SO
import test_evaluate_gpu as TE
import trained_regime as TR

pytestmark = pytest.mark.gpu


def _reference(cfg, lv, frames, state, cand):
    cols = [EO.evaluate(cfg, *lv, frames, state, cand[:, j]) for j in range(cand.shape[1])]
    return {k: np.stack([c[k] for c in cols], -1) for k in ("q", "q_target")}


def _check(label, core, frames, state, cand, ref):
    for key, target in (("q", False), ("q_target", True)):
        got = core.eval_q(frames, TE._dev(state), TE._dev(cand), target=target).cpu().numpy()
        print(label, key, f"{AH.rel_err(got, ref[key]):.2e}")
        assert AH.rel_err(got, ref[key]) < TE.TOL, (label, key)
    assert AH.rel_err(ref["q"], ref["q_target"]) > 1e-3        # (the target copy differs: reading the wrong one shows)


# (id, A, N, n, critic widths, ensemble, LayerNorm, activation).  c1: one plain relu layer, the Q head on the fan-out rows.  c3: six LDS chunks,
# the last short; n * N = 63; a last workgroup with one live wave.  c4: a candidate per register batch, two chunks staged per batch.  c5: one chunk, two batches.
SWEEP = [("c1_one_layer_plain_relu", 1, 1, 1, (64,), 2, False, "relu"), ("c2_four_layers_e10", 5, 3, 5, (256, 64, 128, 64), 10, True, "tanh"),
         ("c3_A64_w320_swish", 64, 7, 9, (320, 64), 2, True, "swish"), ("c4_N65_w1024_plain", 8, 65, 1, (1024, 64), 2, False, "tanh"),
         ("c5_ragged_65_127_swish", 4, 9, 6, (65, 127), 3, True, "swish")]


@pytest.mark.parametrize("case", SWEEP, ids=[c[0] for c in SWEEP])
def test_state_only_against_the_restatement(gpu, case):
    name, A, N, n, dims, ens, ln, act = case
    cfg = PF.FixedConfig(image_keys=(), discount=0.99, S=10, A=A, hidden=dims[0], ensemble=ens, critic_dims=dims, policy_dims=(64,),
                         critic_layer_norm=ln, critic_activation=act)
    rng = np.random.default_rng(5)
    state, cand = rng.standard_normal((n, cfg.S)).astype(np.float32), EO.scaled_actions(rng.uniform(-1, 1, (n, N, A)))
    with MR.installed(), MP.relu_margin() as margins:
        trunk, theta = PF.init_params(cfg, 42)
        target = TR.perturb_target(theta, cfg) if "critic/w2" in theta else {**theta, "critic/w1": theta["critic/w1"] * np.float32(0.9)}
        ref = _reference(cfg, (trunk, theta, target), {}, state, cand)
        core = AH.load_leaves(MR.make_core(cfg, n * N), cfg, trunk, theta, target)
    assert bool(margins) == (act == "relu") and all(m >= MP.RELU_MARGIN for m in margins), margins
    _check(name, core, None, state, cand, ref)


def test_frozen_trunk_camera_against_the_restatement(gpu):
    cfg, n, _ = EO.GOLDEN["drq_one_cam"]
    lv, pb = EO.leaves(cfg), EO.golden_inputs("drq_one_cam")
    frames = {k: v[:, 0] for k, v in pb["frames"].items()}
    cand = EO.scaled_actions(np.random.default_rng(6).uniform(-1, 1, (n, 3, cfg.A)))
    _check("drq_one_cam N=3", TE._core(cfg, 3 * n, lv), TE._dev(np.stack([frames[k] for k in cfg.image_keys])), pb["state"][:, 0], cand,
           _reference(cfg, lv, frames, pb["state"][:, 0], cand))


def test_small_encoder_stack_of_two_against_the_restatement(gpu):
    T, n, cfg = 2, 7, SO.config(keys=("wrist",), H=32, W=32, S=5, A=3, T=2, ensemble=3)
    theta = {k: np.asarray(v, np.float32) for k, v in SO.init_params(cfg, T).items()}
    target = TR.perturb_target(theta, cfg)
    _, core = SO.make_pair(cfg, T, 3 * n)
    for sec, th in (("params", theta), ("target_params", target)):
        core.load_flat(sec, {SO.product_name(k, cfg.image_keys): v for k, v in th.items()})
    rng = np.random.default_rng(8)
    frames = rng.integers(0, 256, (n, T, cfg.H, cfg.W, 3), dtype=np.uint8)
    state, cand = rng.standard_normal((n, cfg.S)).astype(np.float32), EO.scaled_actions(rng.uniform(-1, 1, (n, 3, cfg.A)))
    _check("small T=2 N=3", core, TE._dev(frames[None]), state, cand, _reference(cfg, ({}, theta, target), {"wrist": SO.fold(frames)}, state, cand))


def test_columns_equal_the_one_action_call_and_equal_candidates_equal_bits(gpu, target=True):
    cfg, n = TE._state_cfg(5, 256, 2), 3
    core = TE._core(cfg, 32, TE._leaves(cfg, "init"))
    rng = np.random.default_rng(9)
    state, cand = TE._dev(rng.standard_normal((n, cfg.S)).astype(np.float32)), EO.scaled_actions(rng.uniform(-1, 1, (n, 10, cfg.A)))
    cand[:, 2] = cand[:, 9] = cand[:, 0]          # the same candidate twice in a register batch of eight, and once in the next
    cand = TE._dev(cand)
    single = [core.eval_q(None, state, cand[:, j].contiguous(), target).cpu().numpy() for j in range(7)]
    one, four = (core.eval_q(None, state, cand[:, c].contiguous(), target).cpu().numpy() for c in (slice(0, 1), slice(3, 7)))   # (another order of sums: no bits)
    assert AH.rel_err(one[..., 0], single[0]) < TE.TOL and all(AH.rel_err(four[..., j], single[3 + j]) < TE.TOL for j in range(4))
    ten = core.eval_q(None, state, cand, target).cpu().numpy()
    assert np.array_equal(ten[..., 0], ten[..., 2]) and np.array_equal(ten[..., 0], ten[..., 9]) and not np.array_equal(ten[..., 0], ten[..., 1])


def test_python_surface_chunks_and_refusals(gpu):
    from serl_amd._lib import SerlError, check
    cfg, agent = TE._golden_agent("sac_state", B=8)
    rng = np.random.default_rng(4)
    state, cand = rng.standard_normal((7, cfg.S)).astype(np.float32), EO.scaled_actions(rng.uniform(-1, 1, (7, 3, cfg.A)))
    for target in (False, True):
        whole = agent.q_values(state, cand, target=target)           # 8 // 3 = 2 observations per call: four calls
        assert whole.shape == (cfg.ensemble, 7, 3) and whole.dtype == np.float32
        for lo, hi in ((0, 2), (2, 4), (4, 6), (6, 7)):
            assert np.array_equal(agent.q_values(state[lo:hi], cand[lo:hi], target=target), whole[:, lo:hi]), (target, lo)
    for bad, message in ((cand[:5], "7 observations"), (np.zeros((7, 9, cfg.A), np.float32), "batch_size")):
        with pytest.raises(ValueError, match=message):
            agent.q_values(state, bad)
    core, s, a = agent.core, TE._dev(state), TE._dev(cand)
    with pytest.raises(SerlError, match=r"n \* n_actions = 3 \* 3 not in \[1,8\]"):
        core.eval_q(None, s[:3], a[:3])
    out = torch.empty((cfg.ensemble, 2, 3), device="cuda")
    for args, message in (((2, 0, 0, out.data_ptr()), "n_actions 0 is not positive"), ((2, 3, 0, None), "dev_actions or dev_q_out is NULL")):
        rc = core.L.serl_agent_eval_q_actions(core._h, None, s.data_ptr(), a.data_ptr(), *args, None)
        assert rc == -1                                                # SERL_ERR_INVALID
        with pytest.raises(SerlError, match=message):
            check(rc)


def test_the_calls_leave_the_training_state_bit_identical(gpu):
    rb, agent = TE._store_setup()
    agent.update_high_utd(rb.gather(TE._valid(rb, 0, 8)), utd_ratio=2)         # away from step 0 and from zero moments
    before = TE._state_of(agent)
    obs, act = TE._rows(agent, rb.gather(TE._valid(rb, 16, 19)))
    assert [agent.q_values(obs, np.stack([act, -act], 1), target=t).shape for t in (False, True)] == [(10, 3, 2)] * 2
    torch.cuda.synchronize()
    assert TE._same(before, TE._state_of(agent)) == []
    ends = []       # state-only, and the update that follows: the same with the calls in front of it as without
    for calls in (False, True):
        cfg, sac = TE._golden_agent("sac_state")
        pb = EO.golden_inputs("sac_state")
        sac.update(TE.GR.ref_batch(cfg, pb))
        for target in (False, True) if calls else ():
            sac.q_values(pb["state"][:4, 0], np.stack([pb["action"][:4], pb["action"][4:]], 1), target=target)
        sac.update(TE.GR.ref_batch(cfg, pb))
        ends.append(TE._state_of(sac))
    assert TE._same(*ends) == []
