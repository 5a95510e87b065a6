"""GPU: acting on the critic -- N policy samples per observation ranked by Q: sample_actions(num_candidates=) / policy_samples /
AgentCore.sample_best over serl_agent_sample_candidates, serl_agent_sample_best, policy_fanout_kernel and q_rank_kernel (heads.hip).
Without the feature every test fails at its first call: the keyword, the method and the symbols are missing.  Reference: mean and
std from tests/eval_oracle.py::evaluate in fp64; the candidates and their log-density are the float64 lines of _reference; Q per
candidate column from evaluate again, as in tests/test_q_actions_gpu.py.  Bounds (absolute): candidates, Q and score TOL = 1e-4,
log-density 1e-4 max(1, |ref|); the chosen candidate's oracle score within 2 TOL max(1, |max|) of the oracle's maximum in every
row, and the oracle's index wherever its own top-two gap is at least 1e-3 (at least three quarters of every case's rows, asserted
on the oracle alone before the GPU's answer is read).  Measured worst on an MI355X: candidates 9.9e-7 (c4), Q 1.8e-5 and score
1.6e-5 (the frozen trunk and c7, where |Q| is about 100; 1.0e-6 elsewhere), log-density 3.4e-6 (c3); every row of every case clear."""
import numpy as np
import pytest
import torch

import agent_helpers as AH
import eval_oracle as EO
import mlp_ragged as MR
import policy_fixed as PF
import stacked_oracle as SO
import test_evaluate_gpu as TE
import trained_regime as TR

pytestmark = pytest.mark.gpu
GAP = 1e-3


def _reference(cfg, lv, frames, state, eps, rank):
    zero = np.zeros((state.shape[0], cfg.A), np.float32)
    base = EO.evaluate(cfg, *lv, frames, state, zero)
    z = eps.astype(np.float64).transpose(1, 0, 2)                                             # [n, N, A]
    mean, sd = base["mean"][:, None], base["std"][:, None]
    u = mean + sd * z
    lp = -0.5 * z * z - np.log(sd) - 0.5 * np.log(2.0 * np.pi)
    if cfg.tanh_squash:
        lp = lp - 2.0 * (np.log(2.0) - u - np.logaddexp(0.0, -2.0 * u))
    cand = np.tanh(u) if cfg.tanh_squash else u
    with np.errstate(all="ignore"):      # (evaluate's own log_prob of a candidate at +-1 is not finite and not read)
        q = np.stack([EO.evaluate(cfg, *lv, frames, state, cand[:, j])["q"] for j in range(cand.shape[1])], -1)
    return {"actions": cand, "log_prob": lp.sum(-1), "q": q, "score": q.min(0) if rank == "min" else q.mean(0), "std": base["std"]}


def _check(label, core, frames, state, eps, ref, rank, saturated=False):
    n, N = ref["score"].shape
    top = np.sort(ref["score"], 1)[:, ::-1]
    clear = (top[:, 0] - top[:, 1] >= GAP) if N > 1 else np.ones(n, bool)
    assert clear.mean() >= 0.75, (label, clear)                                               # the oracle alone
    got = {k: v.cpu().numpy() for k, v in core.sample_best(frames, TE._dev(state), TE._dev(eps), rank=rank).items()}
    got["log_prob"] = core.sample_candidates(frames, TE._dev(state), TE._dev(eps))["log_prob"].cpu().numpy()
    best = ref["score"].max(1)
    fig = {k: float(np.abs(got[k] - ref[k]).max()) for k in ("actions", "q")}
    fig["score"] = float(np.abs(got["score"] - best).max())
    fig["log_prob"] = EO.row_error(got["log_prob"], ref["log_prob"])
    print(label, {k: f"{v:.2e}" for k, v in fig.items()}, f"clear rows {int(clear.sum())}/{n}")
    assert np.isfinite(got["log_prob"]).all() and all(v < TE.TOL for v in fig.values()), (label, fig)
    chosen = ref["score"][np.arange(n), got["index"]]
    assert (best - chosen <= 2 * TE.TOL * np.maximum(1.0, np.abs(best))).all(), (label, best - chosen)
    assert (got["index"] == ref["score"].argmax(1))[clear].all(), (label, got["index"], ref["score"].argmax(1))
    assert np.array_equal(got["action"], got["actions"][np.arange(n), got["index"]])
    if saturated:      # tanh rounds to +-1 in float32: the log-density of those samples is finite and inside the bound above
        assert (np.abs(got["actions"]) == 1.0).any()


# (id, A, N, n, ensemble, std, squash, regime, rank, hidden, critic dims (ragged: the PF family) or None, fixed std or None).  A: one active
# lane, a partial wave, a full wave.  N = 65: nine register passes of eight with a last candidate alone, and two candidates on lane 0
# of the rank reduction.  c6: n * N = cfg.batch.  c7: whole std columns on both clips and means at +12 / -7 (saturated tanh).
FIXED = (1e-6, 0.3, 7.0, 0.05, 1.0)      # below std_min, inside, above std_max
SWEEP = [("c1_exp_tanh_A5_e10", 5, 3, 5, 10, "exp", True, "init", "min", 256, None, None),
         ("c2_softplus_tanh_A1_N1_n1", 1, 1, 1, 2, "softplus", True, "init", "min", 64, None, None),
         ("c3_uniform_tanh_A64_N65_mean", 64, 65, 1, 2, "uniform", True, "init", "mean", 320, None, None),
         ("c4_exp_gauss_mean", 5, 3, 5, 10, "exp", False, "init", "mean", 256, None, None),
         ("c5_softplus_gauss_N65", 5, 65, 1, 2, "softplus", False, "init", "min", 256, None, None),
         ("c6_uniform_gauss_full_batch", 5, 3, 24, 2, "uniform", False, "init", "min", 64, None, None),
         ("c7_exp_tanh_A8_clipped_saturated", 8, 3, 5, 10, "exp", True, "trained", "mean", 256, None, None),
         ("c8_fixed_std_tanh", 5, 3, 5, 2, "exp", True, "init", "min", 64, (64, 64), FIXED),
         ("c9_ragged_65_127_swish", 4, 9, 6, 3, "exp", True, "init", "min", 65, (65, 127), None)]


@pytest.mark.parametrize("case", SWEEP, ids=[c[0] for c in SWEEP])
def test_state_only_against_the_restatement(gpu, case):
    name, A, N, n, ens, std, squash, regime, rank, hidden, dims, fixed = case
    rng = np.random.default_rng(11)
    state, eps = rng.standard_normal((n, 10)).astype(np.float32), rng.standard_normal((N, n, A)).astype(np.float32)
    if dims is None:
        cfg = TE._state_cfg(A, hidden, ens, std, squash)
        lv = TE._leaves(cfg, regime)
        ref, core = _reference(cfg, lv, {}, state, eps, rank), TE._core(cfg, 72, lv)
    else:
        cfg = PF.FixedConfig(image_keys=(), discount=0.99, S=10, A=A, hidden=hidden, ensemble=ens, critic_dims=dims, policy_dims=(64,),
                             critic_activation="swish", fixed_std=fixed)
        with MR.installed():
            trunk, theta = PF.init_params(cfg, 42)
            pin = (lambda th: PF.pinned_theta(cfg, th)) if fixed else (lambda th: th)
            ref = _reference(PF.pinned_config(cfg) if fixed else cfg, (trunk, pin(theta), pin(theta)), {}, state, eps, rank)
            core = AH.load_leaves(MR.make_core(cfg, 72), cfg, trunk, theta)
    if regime == "trained":
        lo, _, hi = TR.clip_columns(cfg)
        assert (ref["std"][:, lo] == cfg.std_min).all() and (ref["std"][:, hi] == cfg.std_max).all() and len(lo) and len(hi)
    _check(name, core, None, state, eps, ref, rank, saturated=regime == "trained")


def _small_core(n_rows):
    T, cfg = 2, SO.config(keys=("wrist",), H=32, W=32, S=5, A=3, T=2, ensemble=3)
    theta = {k: np.asarray(v, np.float32) for k, v in SO.init_params(cfg, T).items()}
    _, core = SO.make_pair(cfg, T, n_rows)
    core.load_flat("params", {SO.product_name(k, cfg.image_keys): v for k, v in theta.items()})
    return cfg, theta, core


@pytest.mark.parametrize("encoder", ["frozen_trunk_64", "small_stack_of_two_32"])
def test_pixel_agents_against_the_restatement(gpu, encoder):
    rng = np.random.default_rng(12)
    if encoder == "frozen_trunk_64":
        cfg, n, _ = EO.GOLDEN["drq_one_cam"]
        lv, pb = EO.leaves(cfg), EO.golden_inputs("drq_one_cam")
        frames, state = {k: v[:, 0] for k, v in pb["frames"].items()}, pb["state"][:, 0]
        core, dev_frames = TE._core(cfg, 3 * n, lv), np.stack([frames[k] for k in cfg.image_keys])
    else:
        n = 7
        cfg, theta, core = _small_core(3 * n)
        raw = rng.integers(0, 256, (n, 2, cfg.H, cfg.W, 3), dtype=np.uint8)
        lv, frames, dev_frames, state = ({}, theta, theta), {"wrist": SO.fold(raw)}, raw[None], rng.standard_normal((n, cfg.S)).astype(np.float32)
    eps = rng.standard_normal((3, n, cfg.A)).astype(np.float32)
    _check(encoder, core, TE._dev(dev_frames), state, eps, _reference(cfg, lv, frames, state, eps, "min"), "min")


def test_bit_for_bit_invariants_and_read_only(gpu):
    cfg, agent = TE._golden_agent("sac_state", B=8)
    pb = EO.golden_inputs("sac_state")
    agent.update(TE.GR.ref_batch(cfg, pb))                                                    # away from step 0 and from zero moments
    before = TE._state_of(agent)
    state, seed, rows = np.random.default_rng(13).standard_normal((7, cfg.S)).astype(np.float32), np.array([3, 4], np.uint32), np.arange(7)
    assert np.array_equal(agent.sample_actions(state, seed=seed, num_candidates=1), agent.sample_actions(state, seed=seed))
    action, info = agent.sample_actions(state, seed=seed, num_candidates=3, return_info=True)   # 8 // 3 = 2 observations per call: four calls
    assert action.shape == (7, cfg.A) and info["q"].shape == (cfg.ensemble, 7, 3) and info["index"].dtype == np.int32
    assert np.array_equal(action, info["actions"][rows, info["index"]]) and np.array_equal(action, agent.sample_actions(state, seed=seed, num_candidates=3))
    samples = agent.policy_samples(state, seed=seed, num_samples=3)
    assert np.array_equal(info["actions"], samples["actions"]) and samples["log_prob"].shape == (7, 3)
    assert np.array_equal(info["q"], agent.q_values(state, info["actions"]))
    one, one_info = agent.sample_actions(state[0], seed=seed, num_candidates=3, rank="mean", return_info=True)
    assert one.shape == (cfg.A,) and one_info["q"].shape == (cfg.ensemble, 3) and one_info["index"].shape == ()
    core, eps = agent.core, agent._action_noise(seed, 7, 3)
    for lo, hi in ((0, 2), (2, 4), (4, 6), (6, 7)):                                           # chunked == direct, each chunk on its slice of eps
        part = core.sample_best(None, TE._dev(state[lo:hi]), eps[:, lo:hi].contiguous())
        assert all(np.array_equal(part[k].cpu().numpy(), info[k][:, lo:hi] if k == "q" else (action if k == "action" else info[k])[lo:hi]) for k in part)
    eps[2] = eps[0]                                                                           # equal eps rows: equal bits, wherever they stand
    twin = core.sample_candidates(None, TE._dev(state[:2]), eps[:, :2].contiguous())
    assert all(torch.equal(v[:, 0], v[:, 2]) and not torch.equal(v[:, 0], v[:, 1]) for v in twin.values())
    same = core.sample_best(None, TE._dev(state[:2]), eps[:1, :2].expand(3, 2, cfg.A).contiguous())
    assert same["index"].tolist() == [0, 0]                                                   # all N equal: ties go to the lowest index
    torch.cuda.synchronize()
    assert TE._same(before, TE._state_of(agent)) == []


def test_refusals(gpu):
    from serl_amd._lib import SerlError
    cfg, agent = TE._golden_agent("sac_state", B=8)
    s, eps = torch.zeros((3, cfg.S), device="cuda"), torch.zeros((3, 3, cfg.A), device="cuda")
    for call in (agent.core.sample_best, agent.core.sample_candidates):
        with pytest.raises(SerlError, match=r"n \* n_cand = 3 \* 3 not in \[1,8\]"):
            call(None, s, eps)
    for kw, message in ((dict(argmax=True, num_candidates=2), "argmax"), (dict(seed=1, num_candidates=2, rank="max"), "rank"),
                        (dict(seed=1, num_candidates=9), "batch_size")):
        with pytest.raises(ValueError, match=message):
            agent.sample_actions(s.cpu().numpy(), **kw)


def test_one_call_launches_one_encoder_and_fewer_kernels_than_the_composition(gpu):
    n, N = 4, 3
    cfg, _, core = _small_core(n * N)
    rng = np.random.default_rng(14)
    frames = TE._dev(rng.integers(0, 256, (1, n, 2, cfg.H, cfg.W, 3), dtype=np.uint8))
    state, eps = TE._dev(rng.standard_normal((n, cfg.S)).astype(np.float32)), TE._dev(rng.standard_normal((N, n, cfg.A)).astype(np.float32))
    cand = core.sample_candidates(frames, state, eps)["actions"]

    def launches(call):
        n0 = core.L.serl_debug_chain_launches()
        call()
        return int(core.L.serl_debug_chain_launches() - n0)
    best = launches(lambda: core.sample_best(frames, state, eps, info=False))
    policy, q = launches(lambda: core.eval_policy(frames, state)), launches(lambda: core.eval_q(frames, state, cand))
    encoder = q - 2 * len(core.critic_dims)      # (a critic layer is a GEMM and a row kernel; the rest of the call is the encoder)
    print("launches", {"sample_best": best, "eval_policy": policy, "eval_q_actions": q, "encoder": encoder})
    assert encoder >= 4 and best < policy + q                                                  # the SmallEncoder's GEMMs and the two heads
    assert best == policy + q - encoder + 1                                                    # one encoder's launches, not two; + q_rank_kernel
