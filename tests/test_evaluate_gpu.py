"""GPU: read-only evaluation -- DrQAgent / SACAgent.q_values, policy_stats, evaluate_batch, evaluate_losses over
serl_agent_eval_q / serl_agent_eval_policy / serl_agent_eval_losses and policy_stats_kernel (heads.hip).

Without the feature every test here fails at its first evaluation call (AttributeError / a missing symbol).

  * against the fp64 restatement (tests/eval_oracle.py) at TOL = 1e-4 of tests/test_agent_gpu.py under AH.rel_err for q, q_target,
    mean, std, mode; log_prob within max(1e-4, 4 x the fp32 restatement's own error) per row, normalised by max(1, |ref|) -- the
    bound tests/test_trained_regime_gpu.py uses for the policy head (the factor covers the K-split order of the head GEMM and the
    lane-order reduction);
  * against the reference's recorded answers (tests/golden/eval_*.npz) with leaf_compare and the 1e-4 of
    tests/test_golden_update_gpu.py;
  * bit-level invariants: mode == sample_actions(argmax=True), std == the update's own std, chunked == direct, LazyBatch == dict;
  * read-only: parameters, targets, moments, step and state.rng bit-identical after every call, and a run with evaluation calls
    between its updates ends bit-identical to one without, reward labels included;
  * evaluate_losses: within TOL of the oracle's losses and bit-identical to the info of the update that follows, in both chain modes;
  * the refusals and one raw-pointer call of each C entry.

Measured worst errors on an MI355X, over all cases of section 1 (bound 1e-4 each): q 2.8e-6, q_target 1.5e-6, mean 4.9e-7,
std 4.3e-7, mode 6.6e-7; log_prob 1.3e-6 per row (softplus + tanh, A = 1, n = 64) beside that case's fp32 restatement at 1.4e-6 --
the worst fp32 yardstick of any case is 1.8e-6, so the bound is its floor of 1e-4 everywhere.  Against the goldens: q 1.9e-7,
q_target 1.3e-7, mean / std / mode 1.1e-7, log_prob 2.1e-7.  evaluate_losses against the oracle: worst 1.0e-6 (entropy, one camera)."""
import ctypes as C
import dataclasses
import itertools

import numpy as np
import pytest
import torch

from oracle import drq_oracle as O
from oracle import golden_update as G
import agent_helpers as AH
import eval_oracle as EO
import golden_replay as GR
import policy_modes as PM
import stacked_oracle as SO
import trained_regime as TR

pytestmark = pytest.mark.gpu
TOL = 1e-4           # tests/test_agent_gpu.py
ROWS = (1, 5, 64, 65, 72)      # four rows per workgroup of policy_stats_kernel, 64-row GEMM tiles, cfg.batch itself
FIVE = ("q", "q_target", "mean", "std", "mode")


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), device="cuda")


def _state_cfg(A, hidden, ensemble, std="exp", squash=True):
    return PM.mode_config(std, squash, image_keys=(), S=10, A=A, ensemble=ensemble, discount=0.99, hidden=hidden, warmup=4, temp_warmup=0)


def _leaves(cfg, regime):
    """-> (trunk, theta, target): "init" = O.init_params (std in its usual range, nothing clips), "trained" = whole std columns on
    both clips (trained_regime.clip_columns); the target copy differs in both"""
    trunk, theta = O.init_params(dataclasses.replace(cfg, std_parameterization="exp"), 42)
    theta = PM.mode_theta(theta, cfg, cfg.std_parameterization, regime)       # "trained": policy_modes.CLIP_CYCLE clips exp and softplus on both sides
    return trunk, theta, TR.perturb_target(theta, cfg)


def _core(cfg, B, leaves, fuse=None):
    trunk, theta, target = leaves
    return AH.load_leaves(AH.make_core(cfg, B, fuse=fuse), cfg, trunk, theta, target)


def _check(label, got, ref64, err32):
    """the five quantities at TOL, log_prob per row at max(1e-4, 4 x the fp32 restatement's error); prints every figure first"""
    fig = {q: AH.rel_err(got[q], ref64[q]) for q in FIVE}
    fig["log_prob"] = EO.row_error(got["log_prob"], ref64["log_prob"])
    bound = max(1e-4, 4.0 * err32)
    print(label, {k: f"{v:.2e}" for k, v in fig.items()}, f"log_prob fp32 yardstick {err32:.2e} bound {bound:.2e}")
    for q in FIVE:
        assert fig[q] < TOL, (label, q, fig[q])
    assert np.isfinite(got["log_prob"]).all() and fig["log_prob"] <= bound, (label, fig["log_prob"], bound)


def _core_eval(core, frames, state, actions):
    out = {"q": core.eval_q(frames, state, actions), "q_target": core.eval_q(frames, state, actions, target=True),
           **core.eval_policy(frames, state, actions)}
    return {k: v.cpu().numpy() for k, v in out.items()}


# ---- 1. against the fp64 restatement ------------------------------------------------------------------------------------------
# (id, A, ensemble, hidden, std, squash, regime): A in {1, 5, 64}; ensembles 2 and 10; widths 64 / 256 / 320 = the three LayerNorm row
# layouts; all six std x squash modes; two cases with whole std columns clipped
SWEEP = [
    ("exp_tanh_A5_e10_w256", 5, 10, 256, "exp", True, "init"),
    ("softplus_tanh_A1_e2_w64", 1, 2, 64, "softplus", True, "init"),
    ("uniform_tanh_A64_e2_w320", 64, 2, 320, "uniform", True, "init"),
    ("exp_gauss_A5_e10_w256", 5, 10, 256, "exp", False, "init"),
    ("softplus_gauss_A5_e2_w256", 5, 2, 256, "softplus", False, "init"),
    ("uniform_gauss_A5_e2_w64", 5, 2, 64, "uniform", False, "init"),
    ("exp_tanh_A8_e10_w256_clipped", 8, 10, 256, "exp", True, "trained"),
    ("softplus_tanh_A5_e2_w320_clipped", 5, 2, 320, "softplus", True, "trained"),
]


@pytest.mark.parametrize("case", SWEEP, ids=[c[0] for c in SWEEP])
def test_state_only_against_the_restatement(gpu, case):
    name, A, ens, hidden, std, squash, regime = case
    cfg, B = _state_cfg(A, hidden, ens, std, squash), 72
    lv = _leaves(cfg, regime)
    core = _core(cfg, B, lv)
    rng = np.random.default_rng(5)
    state = rng.standard_normal((B, cfg.S)).astype(np.float32)
    act = EO.scaled_actions(rng.uniform(-1, 1, (B, A)))
    ref64, err32 = EO.log_prob_yardstick(cfg, *lv, {}, state, act)       # once, for all row counts (rows are independent)
    if regime == "trained":
        lo, _, hi = TR.clip_columns(cfg)
        assert (ref64["std"][:, lo] == cfg.std_min).all() and (ref64["std"][:, hi] == cfg.std_max).all() and len(lo) and len(hi)
    for n in ROWS:
        got = _core_eval(core, None, _dev(state[:n]), _dev(act[:n]))
        assert got["q"].shape == (ens, n) and got["mean"].shape == (n, A) and got["log_prob"].shape == (n,)
        _check(f"{name} n={n}", got, {k: (v[:, :n] if k in ("q", "q_target") else v[:n]) for k, v in ref64.items()}, err32)
    assert AH.rel_err(ref64["q"], ref64["q_target"]) > 1e-3        # (the target copy differs: reading the wrong one shows)
    if squash:      # a stored action at exactly +-1: that row is not finite, here and in the restatement; its neighbours are
        a1 = act[:5].copy()
        a1[2, 0], a1[4, A - 1] = 1.0, -1.0
        got = core.eval_policy(None, _dev(state[:5]), _dev(a1))["log_prob"].cpu().numpy()
        ref = EO.evaluate(cfg, *lv, {}, state[:5], a1, torch.float64)["log_prob"]
        assert (~np.isfinite(got)).tolist() == (~np.isfinite(ref)).tolist() == [False, False, True, False, True]


def test_one_camera_resnet_against_the_restatement(gpu):
    name = "drq_one_cam"
    cfg, B, _ = EO.GOLDEN[name]
    lv = EO.leaves(cfg)
    core = _core(cfg, B, lv)
    pb = EO.golden_inputs(name)
    frames = {k: v[:, 0] for k, v in pb["frames"].items()}
    ref64, err32 = EO.log_prob_yardstick(cfg, *lv, frames, pb["state"][:, 0], pb["action"])
    f = _dev(np.stack([frames[k] for k in cfg.image_keys]))
    for n in (B, 1, 5):
        got = _core_eval(core, f[:, :n].contiguous(), _dev(pb["state"][:n, 0]), _dev(pb["action"][:n]))
        _check(f"{name} n={n}", got, {k: (v[:, :n] if k in ("q", "q_target") else v[:n]) for k, v in ref64.items()}, err32)


def test_small_encoder_stack_of_two_against_the_restatement(gpu):
    T, B = 2, 7
    cfg = SO.config(keys=("wrist",), H=32, W=32, S=5, A=3, T=T, ensemble=3)
    theta = {k: np.asarray(v, np.float32) for k, v in SO.init_params(cfg, T).items()}
    target = TR.perturb_target(theta, cfg)
    _, core = SO.make_pair(cfg, T, B)
    for sec, th in (("params", theta), ("target_params", target)):
        core.load_flat(sec, {SO.product_name(k, cfg.image_keys): v for k, v in th.items()})
    rng = np.random.default_rng(8)
    frames = rng.integers(0, 256, (B, T, cfg.H, cfg.W, 3), dtype=np.uint8)
    state = rng.standard_normal((B, cfg.S)).astype(np.float32)
    act = EO.scaled_actions(rng.uniform(-1, 1, (B, cfg.A)))
    ref64, err32 = EO.log_prob_yardstick(cfg, {}, theta, target, {"wrist": SO.fold(frames)}, state, act)
    for n in (B, 3):
        got = _core_eval(core, _dev(frames[None, :n]), _dev(state[:n]), _dev(act[:n]))
        _check(f"small T=2 n={n}", got, {k: (v[:, :n] if k in ("q", "q_target") else v[:n]) for k, v in ref64.items()}, err32)


# ---- 2. against the reference's recorded answers --------------------------------------------------------------------------------
def _golden_agent(name, B=None):
    cfg, rows, (std, squash) = EO.GOLDEN[name]
    agent = GR.reference_agent(cfg, B or rows, policy_kwargs=PM.policy_kwargs(std, squash))
    AH.load_leaves(agent.core, cfg, *EO.leaves(cfg))
    return cfg, agent


def _golden_obs(cfg, pb, rows=slice(None)):
    if cfg.state_only:
        return pb["state"][rows, 0]
    return {**{k: v[rows, :1] for k, v in pb["frames"].items()}, "state": pb["state"][rows]}


@pytest.mark.parametrize("name", sorted(EO.GOLDEN))
def test_python_surface_against_the_reference_goldens(gpu, name):
    z = np.load(EO.golden_path(name))
    cfg, agent = _golden_agent(name)
    pb = EO.golden_inputs(name)
    obs = _golden_obs(cfg, pb)
    got = {"q": agent.q_values(obs, pb["action"]), "q_target": agent.q_values(obs, pb["action"], target=True),
           **agent.policy_stats(obs, pb["action"])}
    assert set(got) == set(EO.QUANTITIES)
    for q in EO.QUANTITIES:
        e, how = G.leaf_compare(q, {"full": z[f"{q}/full"]}, got[q])
        print(name, q, f"{e:.2e}")
        assert e < GR.TOL, (q, how, e)
    assert set(agent.policy_stats(obs)) == {"mean", "std", "mode"}                      # no actions: no log_prob
    one = agent.policy_stats(_golden_obs(cfg, pb, 0) if cfg.state_only else {k: v[0] for k, v in obs.items()}, pb["action"][0])
    assert one["mean"].shape == (cfg.A,) and one["log_prob"].shape == ()                # a single observation drops the row axis
    assert AH.rel_err(one["mean"], got["mean"][0]) < TOL


# ---- 3. bit-level invariants ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sac_state", "drq_one_cam", "sac_state_softplus_gauss"])
def test_mode_is_the_argmax_action_bit_for_bit(gpu, name):
    cfg, agent = _golden_agent(name)
    pb = EO.golden_inputs(name)
    obs = _golden_obs(cfg, pb)
    assert np.array_equal(agent.policy_stats(obs)["mode"], agent.sample_actions(obs, argmax=True))


@pytest.mark.parametrize("std,squash", [("exp", True), ("softplus", False), ("uniform", True)])
def test_std_is_the_std_of_an_update_on_the_same_rows_bit_for_bit(gpu, std, squash):
    cfg, B = _state_cfg(5, 256, 2, std, squash), 9
    lv = _leaves(cfg, "trained")
    core = _core(cfg, B, lv)
    b = AH.synth_batch(cfg, B, seed=2)
    db = AH.batch_to_device(cfg, b)
    mine = core.eval_policy(None, db.state[0], None)["std"].cpu().numpy()
    core.update(db, ("actor",), AH.noise_to_device(cfg, O.make_noise(cfg, B, seed=3)))     # its policy evaluation: obs, old parameters
    assert np.array_equal(mine.reshape(-1), core.debug("std", B * cfg.A))
    assert (mine == cfg.std_min).any() and (mine == cfg.std_max).any()


def test_chunked_path_equals_direct_calls_bit_for_bit(gpu):
    name = "sac_state"
    cfg, agent = _golden_agent(name, B=8)
    rng = np.random.default_rng(4)
    state = rng.standard_normal((19, cfg.S)).astype(np.float32)
    act = EO.scaled_actions(rng.uniform(-1, 1, (19, cfg.A)))
    whole = {"q": agent.q_values(state, act), "q_target": agent.q_values(state, act, target=True), **agent.policy_stats(state, act)}
    assert whole["q"].shape == (cfg.ensemble, 19) and whole["log_prob"].shape == (19,)
    for lo, hi in ((0, 8), (8, 16), (16, 19)):
        part = {"q": agent.q_values(state[lo:hi], act[lo:hi]), "q_target": agent.q_values(state[lo:hi], act[lo:hi], target=True),
                **agent.policy_stats(state[lo:hi], act[lo:hi])}
        for q in EO.QUANTITIES:
            assert np.array_equal(part[q], whole[q][:, lo:hi] if q in ("q", "q_target") else whole[q][lo:hi]), (q, lo)


KEYS, SS, SA = ("front", "wrist"), 7, 4


def _store_setup(B=8, seed=3):
    from helpers import make_spaces
    from serl_amd.utils.launcher import make_drq_agent, make_replay_buffer
    from serl_amd.utils.synthetic import transition_stream

    class Env:
        observation_space, action_space = make_spaces(KEYS, 64, 64, 3, 1, SS, SA)
    rb = make_replay_buffer(Env(), capacity=300, type="memory_efficient_replay_buffer", image_keys=KEYS)
    rb.seed(0)
    for tr in itertools.islice(transition_stream(KEYS, 64, 64, 3, 1, SS, SA, 20, 5), 150):
        rb.insert(tr)
    obs = {"front": np.zeros((1, 64, 64, 3), np.uint8), "wrist": np.zeros((1, 64, 64, 3), np.uint8), "state": np.zeros((1, SS), np.float32)}
    agent = make_drq_agent(seed, obs, np.zeros((SA,), np.float32), image_keys=KEYS, encoder_type="resnet-pretrained", batch_size=B)
    return rb, agent


def _valid(rb, lo, hi):
    return np.nonzero(rb.valid_mask())[0][lo:hi].astype(np.int64)


def test_lazy_batch_equals_the_host_dict_bit_for_bit(gpu):
    from serl_amd.data.data_store import LazyBatch
    rb, agent = _store_setup()
    idx = _valid(rb, 8, 16)
    for side in ("observations", "next_observations"):
        lazy = agent.evaluate_batch(LazyBatch([(rb, idx.copy())]), side=side)
        eager = agent.evaluate_batch(rb.gather(idx.copy()), side=side)
        assert set(lazy) == set(EO.QUANTITIES) and lazy["q"].shape == (10, 8) and lazy["mean"].shape == (8, SA)
        for q in EO.QUANTITIES:
            assert np.array_equal(lazy[q], eager[q], equal_nan=True), (side, q)     # (a stored action at +-1: that row's log_prob is NaN)
        assert np.isfinite(lazy["q"]).all() and np.isfinite(lazy["mean"]).all()
    obs_side = agent.evaluate_batch(LazyBatch([(rb, idx.copy())]))
    assert not np.array_equal(obs_side["q"], lazy["q"])            # the two halves of the packed frames are different observations
    with pytest.raises(ValueError, match="side"):
        agent.evaluate_batch(rb.gather(idx.copy()), side="both")


# ---- 4. read-only -----------------------------------------------------------------------------------------------------------------
SECTIONS = ("params", "target_params") + tuple(f"opt/{tx}/{m}" for tx in ("actor", "critic", "temperature") for m in ("mu", "nu"))


def _state_of(agent):
    """every leaf of params and target_params, all six moment sections over the trainable leaves, step and state.rng"""
    out = {"step": np.int64(agent.core.step), "rng": np.array(agent.state.rng)}
    for leaf, n in agent.core.leaves.items():
        for sec in (SECTIONS[:2] if leaf.startswith("trunk/") else SECTIONS):
            out[f"{sec}:{leaf}"] = agent.core.get(sec, leaf).copy()
    return out


def _same(a, b):
    assert set(a) == set(b)
    return [k for k in a if not np.array_equal(a[k], b[k])]


def _evaluate_everything(agent, rb, idx, order):
    """the four calls on store rows `idx`, in the given order; -> their results"""
    from serl_amd.data.data_store import LazyBatch
    g = rb.gather(idx.copy()) if rb is not None else None
    calls = {
        "q": lambda: agent.q_values(*_rows(agent, g), target=False),
        "qt": lambda: agent.q_values(*_rows(agent, g), target=True),
        "pi": lambda: agent.policy_stats(*_rows(agent, g)),
        "batch": lambda: agent.evaluate_batch(LazyBatch([(rb, idx.copy())]), side="next_observations"),
        "losses": lambda: agent.evaluate_losses(LazyBatch([(rb, idx.copy())])),
    }
    return [calls[k]() for k in order]


def _rows(agent, g):
    """host observations and actions of a gathered (packed) sample"""
    obs = {k: g["observations"][k][:, :1].cpu().numpy() for k in KEYS}
    obs["state"] = g["observations"]["state"].cpu().numpy()
    return obs, np.clip(g["actions"].cpu().numpy(), -EO.ACTION_BOUND, EO.ACTION_BOUND)


def test_every_call_leaves_the_training_state_bit_identical(gpu):
    rb, agent = _store_setup()
    agent.update_high_utd(rb.gather(_valid(rb, 0, 8)), utd_ratio=2)         # away from step 0 and from zero moments
    torch.cuda.synchronize()
    before = _state_of(agent)
    for order in (("q", "pi", "losses", "batch", "qt"), ("losses", "batch", "pi", "qt", "q", "losses")):
        res = _evaluate_everything(agent, rb, _valid(rb, 16, 24), order)
        assert all(r is not None for r in res)
        torch.cuda.synchronize()
        assert _same(before, _state_of(agent)) == [], order
    # state-only: the same, through SACAgent
    cfg, sac = _golden_agent("sac_state")
    pb = EO.golden_inputs("sac_state")
    batch = GR.ref_batch(cfg, pb)
    sac.update(batch)
    before = _state_of(sac)
    sac.q_values(pb["state"][:, 0], pb["action"], target=True), sac.policy_stats(pb["state"][:, 0], pb["action"])
    sac.evaluate_losses(batch), sac.evaluate_batch(batch, side="next_observations"), sac.q_values(pb["state"][:, 0], pb["action"])
    assert _same(before, _state_of(sac)) == []


@pytest.mark.parametrize("classifier", [False, True], ids=["plain", "reward_classifier"])
def test_a_run_with_evaluation_calls_between_its_updates_ends_where_one_without_does(gpu, classifier):
    """update_critics -> update_high_utd -> update_critics on lazy batches of the iterator, prefetch on.  The device is drained
    between calls so that every frozen-trunk pass of either agent runs as it would alone (the fused GroupNorm path is claimed by
    one pass at a time per process: tests/test_reward_labels_gpu.py)."""
    from serl_amd.data.data_store import LazyBatch
    runs = []
    for with_eval in (False, True):
        rb, agent = _store_setup()
        rb.seed(0)
        assert agent.prefetch
        if classifier:
            from test_reward_labels_gpu import _store_classifier
            agent.set_reward_classifier(_store_classifier(agent, rb))
        it = rb.get_iterator(sample_args={"batch_size": 8, "pack_obs_and_next_obs": True, "lazy": True})
        infos, labels = [], []
        for call in range(3):
            batch = next(it)
            torch.cuda.synchronize()
            if call == 1:
                _, info = agent.update_high_utd(batch, utd_ratio=2)
            else:
                _, info = agent.update_critics(batch)
            infos.append(info.resolve())
            if classifier:
                labels.append([x.copy() for x in agent.last_reward_labels()])
            torch.cuda.synchronize()
            if with_eval:
                _evaluate_everything(agent, rb, _valid(rb, 24 + 8 * call, 32 + 8 * call), ("losses", "q", "batch", "pi", "qt"))
                torch.cuda.synchronize()
        assert agent._sched is not None          # the updates ran pipelined
        runs.append((_state_of(agent), infos, labels))
    (s0, i0, l0), (s1, i1, l1) = runs
    assert _same(s0, s1) == []
    assert i0 == i1, (i0, i1)
    for a, b in zip(l0, l1):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- 5. evaluate_losses -------------------------------------------------------------------------------------------------------------
LOSS_CASES = [("state", O.Config(image_keys=(), S=10, A=5, discount=0.99, warmup=4, temp_warmup=0), 12),
              ("one_cam", O.Config(image_keys=("image",), H=64, W=64, S=5, A=3), 6)]


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", LOSS_CASES, ids=[c[0] for c in LOSS_CASES])
def test_losses_match_the_oracle_and_the_update_that_follows(gpu, case, fuse):
    _, cfg, B = case
    st, core = AH.make_pair(cfg, B, fuse=fuse)
    b = AH.synth_batch(cfg, B, seed=6)
    noise = O.make_noise(cfg, B, seed=9)
    tb, tn = AH.batch_to_torch(b, torch.float64), O.noise_to_torch(noise, torch.float64)
    tn["redq_idx"] = np.asarray(noise["redq_idx"]).reshape(-1, cfg.subsample)[0]
    fo, fn = O.features(st, tb["obs"]), O.features(st, tb["next"])
    ci, _ = O.critic_update(st, fo, fn, tb["state"], tb["next_state"], tb["action"], tb["reward"], tb["mask"], tn, apply=False)
    ai, _ = O.actor_temp_update(st, fo, fn, tb["state"], tb["next_state"], tn, apply=False)
    want = {**ci, **ai}
    db, dn = AH.batch_to_device(cfg, b), AH.noise_to_device(cfg, noise)
    step = core.step
    got = core.eval_losses(db, dn)
    for k, v in want.items():
        print(case[0], fuse, k, got[k], v)
        assert abs(got[k] - v) <= TOL * max(1.0, abs(v)), (k, got[k], v)
    assert core.step == step
    again = core.eval_losses(db, dn)
    assert again == got                                               # asking twice changes nothing
    core.update(db, ("actor", "critic", "temperature"), dn)
    info = core.read_info()
    assert core.step == step + 1
    for k in got:
        assert np.float32(got[k]).tobytes() == np.float32(info[k]).tobytes(), (k, got[k], info[k])


def test_evaluate_losses_returns_the_nested_info_of_update(gpu):
    cfg, agent = _golden_agent("sac_state")
    batch = GR.ref_batch(cfg, EO.golden_inputs("sac_state"))
    rng0 = np.array(agent.state.rng)
    ev = agent.evaluate_losses(batch)
    assert np.array_equal(rng0, agent.state.rng)                      # keys derived from state.rng, which does not advance
    assert ev == agent.evaluate_losses(batch, rng=rng0) and ev != agent.evaluate_losses(batch, rng=np.array([1, 2], np.uint32))
    _, info = agent.update(batch)                                     # draws from the same state.rng
    up = info.resolve()
    assert set(ev) == set(up) == {"critic", "actor", "temperature", "actor_lr", "critic_lr", "temperature_lr"}
    assert ev == up, (ev, up)
    assert not np.array_equal(rng0, agent.state.rng)


# ---- 6. refusals and the C ABI ------------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    from serl_amd import _lib
    from serl_amd._lib import SerlError
    cfg, B = _state_cfg(4, 256, 2), 8
    core = _core(cfg, B, _leaves(cfg, "init"))
    s, a = torch.zeros((B + 1, cfg.S), device="cuda"), torch.zeros((B + 1, cfg.A), device="cuda")
    with pytest.raises(SerlError, match=r"n 9 not in \[1,8\]"):
        core.eval_q(None, s, a)
    with pytest.raises(SerlError, match=r"n 9 not in \[1,8\]"):
        core.eval_policy(None, s, a)
    with pytest.raises(SerlError, match=r"n 0 not in \[1,8\]"):
        core.eval_policy(None, s[:0], None)
    lp = torch.zeros((B,), device="cuda")
    rc = core.L.serl_agent_eval_policy(core._h, None, s.data_ptr(), None, B, None, None, None, lp.data_ptr(), None)
    assert rc == -1                                                    # SERL_ERR_INVALID
    with pytest.raises(SerlError, match="dev_logp_out is given and dev_actions is NULL"):
        _lib.check(rc)
    pcfg = O.Config(image_keys=("image",), H=64, W=64, S=5, A=3)
    _, pix = AH.make_pair(pcfg, 4)
    ps, pa = torch.zeros((2, pcfg.S), device="cuda"), torch.zeros((2, pcfg.A), device="cuda")
    with pytest.raises(SerlError, match=r"dev_frames is NULL on an agent with 1 camera"):
        pix.eval_q(None, ps, pa)
    with pytest.raises(SerlError, match=r"dev_frames is NULL on an agent with 1 camera"):
        pix.eval_policy(None, ps, pa)


def test_c_abi_with_raw_device_pointers(gpu):
    from serl_amd import _lib
    from serl_amd._lib_agent import SerlInfo
    cfg, B, n = _state_cfg(4, 256, 2), 8, 5
    lv = _leaves(cfg, "init")
    core = _core(cfg, B, lv)
    L, h = _lib.lib(), core._h
    b = AH.synth_batch(cfg, B, seed=1)
    b["action"] = EO.scaled_actions(b["action"])
    db = AH.batch_to_device(cfg, b)
    q = torch.full((cfg.ensemble, n), np.nan, device="cuda")
    _lib.check(L.serl_agent_eval_q(h, None, db.state.data_ptr(), db.action.data_ptr(), n, 1, q.data_ptr(), None))
    mean, lp = torch.full((n, cfg.A), np.nan, device="cuda"), torch.full((n,), np.nan, device="cuda")
    _lib.check(L.serl_agent_eval_policy(h, None, db.state.data_ptr(), db.action.data_ptr(), n, mean.data_ptr(), None, None,
                                        lp.data_ptr(), None))                       # any output may be NULL
    info = SerlInfo()
    _lib.check(L.serl_agent_eval_losses(h, C.byref(db.cstruct), None, C.byref(info), None))
    torch.cuda.synchronize()
    ref = EO.evaluate(cfg, *lv, {}, b["state"][:n], b["action"][:n], torch.float64)
    assert AH.rel_err(q.cpu().numpy(), ref["q_target"]) < TOL and AH.rel_err(mean.cpu().numpy(), ref["mean"]) < TOL
    assert EO.row_error(lp.cpu().numpy(), ref["log_prob"]) < TOL
    assert all(np.isfinite(getattr(info, f)) for f, _ in SerlInfo._fields_)
    assert info.critic_lr == 0.0 and info.temperature_lr == np.float32(cfg.lr)      # step 0: inside the warm-up of 4, none for the temperature
    assert core.step == 0
