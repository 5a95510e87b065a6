"""GPU: the policy head with a fixed standard deviation (serl_agent_create_fixed_std; std_parameterization="fixed" with fixed_std,
actor_critic_nets.py:189-192,212; the kPolFixed instantiations of the head kernels in serl_amd/csrc/heads.hip) on the case table
of tests/policy_fixed.py.

* parity of update_critics and update_high_utd (UTD 1 and the case's) in both schedules of the chain against the fp64 statement
  (the oracle in "uniform" with actor/log_stds pinned, tests/policy_fixed.py): info scalars, q, target_q, next log-prob, every
  gradient leaf, the state after the step, at the tolerances of tests/test_agent_gpu.py (TOL = 1e-4, _compare_state); the pinned
  leaf is in no comparison, and a fixed agent has no such leaf;
* a fixed agent with fixed_std = 1 against the uniform agent whose log_stds is zeros: the read-only calls, everything forward, the
  critic's gradient and dx of one update_critics and one actor phase byte for byte -- expf(0) == 1 exactly, both heads have one
  GEMM group with the same K-splits, and actor/log_stds is the LAST leaf of the actor's range, so every shared leaf of the two
  agents stands at the same arena offset (only temp/lagrange behind it moves by A floats, and Adam is elementwise).  The actor's
  gradient is byte-equal without tanh and within TOL with it: one FMA contraction differs between the two instantiations of
  policy_dist_bwd_kernel (test_gradients_and_state_against_the_uniform_twin says where);
* the reference's own update code (tests/golden/fixed_*.npz);
* the fused chain against the one-launch-per-operation chain bit for bit; the launch count against the uniform agent's;
* serl_agent_fixed_std, a scalar against its vector, a checkpoint round trip and both refusals, two shards against the full batch."""
import numpy as np
import pytest
import torch

from oracle import drq_oracle as O
import agent_helpers as AH
import golden_replay as GR
import mlp_widths as MW
import policy_fixed as PF
import policy_modes as PM
from test_agent_gpu import TOL, _compare_state
from test_chain_fusion_gpu import _assert_state_bits, _bits_equal, _launches
from test_evaluate_gpu import _same, _state_of
from test_mlp_widths_gpu import _Figures, _all_bits, _flat_batch, _info

pytestmark = pytest.mark.gpu
FUSE = pytest.mark.parametrize("fuse", [True, False], ids=["fused", "unfused"])


@pytest.fixture(autouse=True)
def _general_oracle():
    with PF.installed():
        yield


def _core_of(run, fuse):
    """a fresh fixed agent holding the parameters the case's oracle run started from"""
    cfg = run["cfg"]
    trunk, theta = PF.init_params(cfg, PF.PARAM_SEED)
    return AH.load_leaves(AH.make_core(cfg, run["B"], fuse=fuse), cfg, trunk, theta)


def _spans(cfg):
    """-> ({leaf: (lo, hi)} of the fixed agent's arena, Pc, Pa0, Pa1): the actor's range ends behind actor/mean/bias"""
    sl, _ = AH.leaf_slices(cfg)
    pc = sl.get("enc/proprio/ln/bias", sl["critic/head/bias"])[1]
    return sl, pc, sl.get("enc/proprio/dense/kernel", sl["actor/w1"])[0], sl["actor/mean/bias"][1]


def _grads(fig, cfg, core, grads, tap):
    """tests/test_mlp_widths_gpu.py::_grads over the fixed agent's own arena, the pinned leaf's gradient left out"""
    sl, pc, pa0, pa1 = _spans(cfg)
    lo0 = 0 if tap == "g_critic" else pa0
    g = core.debug(tap, pc if tap == "g_critic" else pa1 - pa0)
    seen = 0
    for k, gv in PF.unpinned(grads).items():
        lo, hi = sl[k]
        fig.add(f"{tap} {k}", AH.rel_err(g[lo - lo0:hi - lo0], gv.numpy().reshape(-1)))
        seen += 1
    assert seen >= 4, seen


def _no_std_leaf(core):
    assert not any("logstd" in k or "log_stds" in k for k in core.leaves), list(core.leaves)
    assert [k for k in core.leaves if not k.startswith("trunk/")][-2:] == ["actor/mean/bias", "temp/lagrange"]


# ---- parity against the fp64 statement -----------------------------------------------------------------------------------------
@FUSE
@pytest.mark.parametrize("name", PF.IDS)
def test_update_critics_matches_the_pinned_oracle(gpu, name, fuse):
    run = PF.oracle_run(name, "critics")
    cfg, B, st, aux = run["cfg"], run["B"], run["state"], run["aux"]
    assert run["pin"]["evaluations"] == 1 and run["pin"]["std_err"] <= PF.STD_TOL
    core = _core_of(run, fuse)
    _no_std_leaf(core)
    assert np.array_equal(core.fixed_std, np.asarray(cfg.fixed_std, np.float32))
    core.update_critics(AH.batch_to_device(cfg, run["batch"]), AH.noise_to_device(cfg, run["noise"]))
    fig = _Figures(f"update_critics {name} {'fused' if fuse else 'unfused'}")
    _info(fig, core.read_info(), run["info"], ("critic_loss", "predicted_qs", "target_qs"))
    fig.add("q", AH.rel_err(core.debug("q", cfg.ensemble * B).reshape(cfg.ensemble, B), aux["q"].numpy()))
    fig.add("target_q", AH.rel_err(core.debug("target_q", B), aux["target_q"].numpy()))
    fig.add("next logp", AH.rel_err(core.debug("logp", B), aux["next_logp"].numpy()))
    _grads(fig, cfg, core, aux["grads"], "g_critic")
    fig.check()
    _compare_state(cfg, PF.compared_state(st), core)
    assert core.step == st.step == 1
    assert core.debug("ctr_nonzero", 1)[0] == 0


_UTD = [(n, 1) for n in PF.IDS] + [(n, PF.CASES[n]["utd"]) for n in PF.IDS if PF.CASES[n]["utd"] > 1]


@FUSE
@pytest.mark.parametrize("name,utd", _UTD, ids=[f"{n}-utd{u}" for n, u in _UTD])
def test_update_high_utd_matches_the_pinned_oracle(gpu, name, utd, fuse):
    run = PF.oracle_run(name, ("high_utd", utd))
    cfg, B, st = run["cfg"], run["B"], run["state"]
    assert B % utd == 0 and run["pin"]["evaluations"] == utd + 2 and run["pin"]["std_err"] <= PF.STD_TOL
    assert np.abs(run["aux"]["g_actor"][PF.LEAF].numpy()).min() > 0       # the oracle's own log_stds gradient: a uniform agent would step
    core = _core_of(run, fuse)
    core.update_high_utd(AH.batch_to_device(cfg, run["batch"]), utd, AH.noise_to_device(cfg, run["noise"]))
    fig = _Figures(f"update_high_utd({utd}) {name} {'fused' if fuse else 'unfused'}")
    _info(fig, core.read_info(), run["info"], ("critic_loss", "predicted_qs", "target_qs", "actor_loss", "temperature", "entropy", "temperature_loss"))
    _grads(fig, cfg, core, run["aux"]["g_actor"], "g_actor")
    # the std of the actor phase's own policy evaluation is clip(fixed_std) in every row, in float32
    std = core.debug("std", B * cfg.A).reshape(B, cfg.A)
    want = np.clip(np.asarray(cfg.fixed_std, np.float32), np.float32(cfg.std_min), np.float32(cfg.std_max))
    assert np.array_equal(std, np.broadcast_to(want, std.shape)), (std[0], want)
    fig.check()
    _compare_state(cfg, PF.compared_state(st), core, steps=utd + 1)
    assert core.step == st.step == utd + 1
    assert core.debug("ctr_nonzero", 1)[0] == 0


# ---- fused against un-fused chain ----------------------------------------------------------------------------------------------
def _pair_launches(core, cfg, B, b, noise):
    db, dn = AH.batch_to_device(cfg, b), AH.noise_to_device(cfg, noise)
    torch.cuda.synchronize()
    l0 = _launches()
    core.update_critics(db, dn)
    core.update_high_utd(db, 1, dn)
    torch.cuda.synchronize()
    return _launches() - l0


@pytest.mark.parametrize("name", ["a_state_two_columns_clipped", "b_state_gauss_backup_entropy", "e_frozen_one_camera"])
def test_fused_chain_is_bit_identical_to_the_unfused_chain(gpu, name):
    cfg, B, _ = PF.case_config(name)
    fused, unfused = PF.make_pair(cfg, B, fuse=True)[1], PF.make_pair(cfg, B, fuse=False)[1]
    _, pc, pa0, pa1 = _spans(cfg)
    n_pair = {}
    for it in range(2):
        b = AH.synth_batch(cfg, B, seed=300 + it)
        noise = O.make_noise(cfg, B, seed=400 + it, utd_ratio=1)
        for which, core in (("fused", fused), ("unfused", unfused)):
            n_pair[which] = _pair_launches(core, cfg, B, b, noise)
        for tap, n in (("g_critic", pc), ("g_actor", pa1 - pa0), ("scalars", 8), ("q", cfg.ensemble * B), ("target_q", B), ("logp", B),
                       ("std", B * cfg.A), ("dx", B * (cfg.enc_dim + cfg.A))):
            assert _bits_equal(fused.debug(tap, n), unfused.debug(tap, n)), (name, it, tap)
        fi, pi = fused.read_info(), unfused.read_info()
        assert fi == pi, (name, it, fi, pi)
        _assert_state_bits(cfg, fused, unfused, (name, it))
    print(f"{name}: chain launches per update_critics + update_high_utd(1): fused {n_pair['fused']}, one-per-operation {n_pair['unfused']}")
    assert n_pair["fused"] < n_pair["unfused"], n_pair
    assert fused.debug("ctr_nonzero", 1)[0] == 0


# ---- against the uniform agent, bit for bit ------------------------------------------------------------------------------------
TWIN = dict(image_keys=(), S=10, A=5, discount=0.99)
TWIN_ROWS = 72


def _twin_cores(squash, fuse=None):
    """(fixed core with fixed_std = 1, uniform core with log_stds = 0) holding the same shared leaves; std_min <= 1 <= std_max"""
    uni = O.Config(std_parameterization="uniform", tanh_squash=squash, **TWIN)
    fix = PF.config("state", TWIN["S"], TWIN["A"], 1.0, squash=squash)
    assert uni.std_min <= 1.0 <= uni.std_max and (fix.std_min, fix.std_max) == (uni.std_min, uni.std_max)
    theta = O.init_params(uni, PF.PARAM_SEED)[1]
    assert not theta[PF.LEAF].any()
    a = AH.load_leaves(AH.make_core(fix, TWIN_ROWS, fuse=fuse), fix, None, PF.unpinned(theta))
    b = AH.load_leaves(AH.make_core(uni, TWIN_ROWS, fuse=fuse), uni, None, theta)
    return fix, uni, a, b


LAUNCHES = {}      # (squash, fuse) -> (fixed, uniform): chain launches of update_critics + update_high_utd(1), for the count test below


@FUSE
@pytest.mark.parametrize("squash", [True, False], ids=["tanh", "gauss"])
def test_gradients_and_state_against_the_uniform_twin(gpu, squash, fuse):
    """one update_critics and one actor phase (update_high_utd(1) = one more critic step, then actor + temperature).
    Byte-equal: everything forward (q, target_q, log-probs, std, the loss scalars, every info scalar), the critic's gradient, dx of the
    actor loss, and with them every critic leaf and moment of the state.
    The ACTOR's gradient is byte-equal in the plain Gaussian (G_u = dL/da, no arithmetic) and within TOL under tanh, not byte-equal:
    G_u = dL/da * (1 - a^2) + c_lp * 2a is one source expression in policy_dist_bwd_kernel, but the compiler contracts it into a
    multiply and one FMA in the uniform instantiation and into packed multiplies and an add in the fixed one (which has no std
    branch behind it), so dmean differs by one rounding per element -- measured 1e-7 relative per leaf.  The actor leaves of the
    state then follow at _compare_state's bounds."""
    import types
    fix, uni, a, b = _twin_cores(squash, fuse)
    shared = [k for k in a.leaves]
    assert [k for k in b.leaves if k != PF.LEAF] == shared and b.leaves[PF.LEAF] == fix.A
    sl, pc, pa0, pa1 = _spans(fix)
    batch = AH.synth_batch(fix, TWIN_ROWS, seed=300)
    noise = O.make_noise(fix, TWIN_ROWS, seed=400, utd_ratio=1)
    n = {}
    for which, cfg, core in (("fixed", fix, a), ("uniform", uni, b)):
        n[which] = _pair_launches(core, cfg, TWIN_ROWS, batch, noise)
    LAUNCHES[(squash, fuse)] = (n["fixed"], n["uniform"])
    for tap, cnt in (("g_critic", pc), ("scalars", 8), ("q", fix.ensemble * TWIN_ROWS), ("target_q", TWIN_ROWS),
                     ("logp", TWIN_ROWS), ("std", TWIN_ROWS * fix.A), ("dx", TWIN_ROWS * (fix.enc_dim + fix.A))):
        assert _bits_equal(a.debug(tap, cnt), b.debug(tap, cnt)), (squash, tap)
    ga, gb = a.debug("g_actor", pa1 - pa0), b.debug("g_actor", pa1 - pa0 + fix.A)
    assert np.abs(ga).max() > 0 and (a.debug("std", TWIN_ROWS * fix.A) == 1.0).all()
    g_ls = gb[-fix.A:]
    assert np.abs(g_ls).min() > 0, g_ls           # the twin's own log_stds gradient is there: it has stepped, the fixed agent has not
    assert b.get("params", PF.LEAF).all()
    worst = 0.0
    for k in shared:
        lo, hi = sl[k]
        if not (pa0 <= lo and hi <= pa1):
            continue
        if squash:
            worst = max(worst, AH.rel_err(ga[lo - pa0:hi - pa0], gb[lo - pa0:hi - pa0]))
            assert AH.rel_err(ga[lo - pa0:hi - pa0], gb[lo - pa0:hi - pa0]) < TOL, (k, worst)
        else:
            assert _bits_equal(ga[lo - pa0:hi - pa0], gb[lo - pa0:hi - pa0]), k
    print(f"twins squash={squash} {'fused' if fuse else 'unfused'}: actor gradient leaves, worst relative difference {worst:.2e}")
    assert a.read_info() == b.read_info()
    critic_side = [k for k in shared if sl[k][1] <= pa0] + ["temp/lagrange"]
    _assert_state_bits(fix, a, b, ("twins", squash), leaves=critic_side if squash else shared)
    for sec in ("opt/temperature/mu", "opt/temperature/nu"):
        assert _bits_equal(a.get(sec, "temp/lagrange"), b.get(sec, "temp/lagrange"))
    twin = types.SimpleNamespace(params={k: torch.tensor(b.get("params", k)) for k in shared},
                                 target={k: torch.tensor(b.get("target_params", k)) for k in shared})
    _compare_state(fix, twin, a, steps=3)


@pytest.mark.parametrize("squash", [True, False], ids=["tanh", "gauss"])
def test_read_only_calls_equal_the_uniform_twins_byte_for_byte(gpu, squash):
    """sample_actions (seeded and argmax), policy_stats (loc, scale, mode, log-prob of given actions), q_values, evaluate_batch and
    evaluate_losses of two agents made by create_states from one seed: fixed_std = 1 and "uniform" at its zero initialisation"""
    S, A, B = TWIN["S"], TWIN["A"], TWIN_ROWS
    fixed = PF.sac_agent(1.0, seed=7, B=B, S=S, A=A, squash=squash)
    twin = MW.sac_agent(256, seed=7, B=B, S=S, A=A, policy_kwargs=PM.policy_kwargs("uniform", squash))
    _no_std_leaf(fixed.core)
    assert fixed.config["fixed_std"] == (1.0,) * A and "fixed_std" not in twin.config
    assert not twin.core.get("params", PF.LEAF).any()
    for leaf in fixed.core.leaves:
        assert _bits_equal(fixed.core.get("params", leaf), twin.core.get("params", leaf)), leaf
    rng = np.random.default_rng(4)
    state, act = rng.standard_normal((B, S)).astype(np.float32), rng.uniform(-0.9, 0.9, (B, A)).astype(np.float32)
    batch = _flat_batch(S, A, B, 11)
    before = _state_of(fixed)
    for what, call in (("argmax", lambda ag: ag.sample_actions(state, argmax=True)),
                       ("seeded", lambda ag: ag.sample_actions(state, seed=np.array([0, 5], np.uint32))),
                       ("one row", lambda ag: ag.sample_actions(state[0], argmax=True)),
                       ("q", lambda ag: ag.q_values(state, act)), ("q target", lambda ag: ag.q_values(state, act, target=True))):
        x, y = call(fixed), call(twin)
        assert x.shape == y.shape and _bits_equal(x, y), what
    for what, call in (("policy_stats", lambda ag: ag.policy_stats(state, act)), ("policy_stats, no actions", lambda ag: ag.policy_stats(state)),
                       ("evaluate_batch", lambda ag: ag.evaluate_batch(batch, side="next_observations"))):
        x, y = call(fixed), call(twin)
        assert set(x) == set(y) and all(_bits_equal(x[k], y[k]) for k in x), what
        assert (x["std"] == 1.0).all()
        if not squash:
            assert np.array_equal(x["mode"], x["mean"])
    stats = fixed.policy_stats(state, act)
    assert np.isfinite(stats["log_prob"]).all() and np.array_equal(stats["mode"], fixed.sample_actions(state, argmax=True))
    lx, ly = fixed.evaluate_losses(batch), twin.evaluate_losses(batch)
    assert lx == ly and np.isfinite(lx["actor"]["actor_loss"]), (lx, ly)
    torch.cuda.synchronize()
    assert _same(before, _state_of(fixed)) == []


def test_launch_count_equals_the_uniform_agents(gpu):
    """update_critics + update_high_utd(1) of case (a)'s shape: the fixed agent launches exactly what the uniform agent launches.
    What fixed drops is the second group of ONE job of the phase's deferred column-sum launch (head_bias_grad: the column sums of
    dpre's second slab, the log_stds gradient) and nothing of the head's weight-gradient GEMM, which had one group already: jobs
    and groups inside launches that stay, so no launch goes.  Pinned: 56 fused, 68 one per operation (measured on the MI355X)."""
    for fuse in (True, False):
        if (True, fuse) not in LAUNCHES:
            fix, uni, a, b = _twin_cores(True, fuse)
            batch, noise = AH.synth_batch(fix, TWIN_ROWS, seed=300), O.make_noise(fix, TWIN_ROWS, seed=400, utd_ratio=1)
            LAUNCHES[(True, fuse)] = (_pair_launches(a, fix, TWIN_ROWS, batch, noise), _pair_launches(b, uni, TWIN_ROWS, batch, noise))
    print(f"chain launches per update_critics + update_high_utd(1), (fixed, uniform): fused {LAUNCHES[(True, True)]}, "
          f"one per operation {LAUNCHES[(True, False)]}")
    for fuse in (True, False):
        n_fixed, n_uniform = LAUNCHES[(True, fuse)]
        assert n_fixed == n_uniform, (fuse, n_fixed, n_uniform)
    assert (LAUNCHES[(True, True)][0], LAUNCHES[(True, False)][0]) == PINNED_LAUNCHES


PINNED_LAUNCHES = (56, 68)


# ---- the reference's own code --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PF.GOLDEN))
def test_hip_update_matches_the_reference_golden(gpu, name):
    """tests/test_policy_modes_gpu.py::test_hip_update_matches_the_reference_golden_in_mode on fixed_<name>.npz (injected noise): the
    agent comes from create_states / create_drq with the reference's own policy_kwargs and policy_fixed=True"""
    g, meta, _ = PF.load_golden(name)
    cfg, B = g["cfg"], g["B"]
    agent = PF.reference_agent(cfg, B)
    _no_std_leaf(agent.core)
    assert agent.config["fixed_std"] == tuple(cfg.fixed_std) == tuple(meta["policy_fixed"]["fixed_std"])
    assert np.array_equal(agent.core.fixed_std, np.asarray(cfg.fixed_std, np.float32))
    AH.load_leaves(agent.core, cfg, *PF.initial_leaves(cfg))
    GR.replay(agent, g, label=f"fixed_{name}")
    assert agent.core.debug("ctr_nonzero", 1)[0] == 0


# ---- the vector itself ---------------------------------------------------------------------------------------------------------
def test_fixed_std_reads_back_and_a_scalar_is_its_vector(gpu):
    S, A, B = 10, 5, 8
    vec = [0.01, 0.3, 1.0, 5.0, 0.7]
    agent = PF.sac_agent(vec, seed=3, B=B, S=S, A=A, std_min=0.05, std_max=2.0)
    assert np.array_equal(agent.core.fixed_std, np.asarray(vec, np.float32)) and agent.core.std_parameterization == "fixed"
    assert agent.config["fixed_std"] == tuple(float(np.float32(x)) for x in vec)
    state = np.random.default_rng(2).standard_normal((B, S)).astype(np.float32)
    std = agent.policy_stats(state)["std"]
    assert np.array_equal(std, np.broadcast_to(np.asarray([0.05, 0.3, 1.0, 2.0, 0.7], np.float32), (B, A)))      # the clip is the kernel's
    assert np.array_equal(agent.core.fixed_std, np.asarray(vec, np.float32))                                       # ... the vector as passed
    scalar, vector = PF.sac_agent(0.1, seed=3, B=B, S=S, A=A), PF.sac_agent([0.1] * A, seed=3, B=B, S=S, A=A)
    assert scalar.config == vector.config and np.array_equal(scalar.core.fixed_std, vector.core.fixed_std)
    batch = _flat_batch(S, A, B, 10)
    for ag in (scalar, vector):
        ag.update_high_utd(batch, utd_ratio=2)
    want = _all_bits(vector)
    for key, v in _all_bits(scalar).items():
        assert _bits_equal(v, want[key]), key
    # any other mode under the switch is the agent of the call without it
    with_switch = MW.sac_agent(256, seed=3, B=B, S=S, A=A, policy_kwargs=PM.policy_kwargs("softplus", False), policy_fixed=True)
    without = MW.sac_agent(256, seed=3, B=B, S=S, A=A, policy_kwargs=PM.policy_kwargs("softplus", False))
    assert list(with_switch.core.leaves.items()) == list(without.core.leaves.items()) and with_switch.config == without.config
    assert with_switch.core.fixed_std is None
    want = _all_bits(without)
    for key, v in _all_bits(with_switch).items():
        assert _bits_equal(v, want[key]), key


def test_create_fixed_std_is_the_create_opts_agent_bit_for_bit(gpu):
    """serl_agent_create_fixed_std fills the struct AgentCore hands to serl_agent_create_opts: the same leaf table, and the same
    params, target and optimizer bits after one update_critics and one update_high_utd(2)"""
    import ctypes as C
    import types
    from serl_amd.agents.core import AgentCore

    class OldEntry(AgentCore):
        def _create(self, cfg):
            cd, pd = (C.c_int32 * len(self.critic_dims))(*self.critic_dims), (C.c_int32 * len(self.policy_dims))(*self.policy_dims)
            fs = (C.c_float * cfg.act_dim)(*self.spec.fixed_std)
            return self.L.serl_agent_create_fixed_std(C.byref(cfg), self._std_param, 0 if self.tanh_squash_distribution else 1, *self._acts,
                                                      cd, len(cd), pd, len(pd), int(self.critic_layer_norm), int(self.policy_layer_norm), fs,
                                                      C.byref(self._h))
    B = 8
    cfg = PF.config("state", 10, 4, (0.1, 0.3, 1.0, 0.7), ensemble=2, critic_dims=(64, 64), policy_dims=(64, 64))
    theta = PF.unpinned(O.init_params(PF.pinned_config(cfg), PF.PARAM_SEED)[1])
    kw = dict(encoder_type=cfg.encoder_type, n_cam=0, H=0, W=0, state_dim=cfg.S, act_dim=cfg.A, batch=B, ensemble=cfg.ensemble, hidden=cfg.hidden,
              discount=cfg.discount, tau=cfg.tau, lr=cfg.lr, warmup_steps=cfg.warmup, dropout=cfg.dropout, std_min=cfg.std_min,
              std_max=cfg.std_max, target_entropy=cfg.target_entropy, seed=5, temp_warmup_steps=-1, std_parameterization="fixed",
              fixed_std=np.asarray(cfg.fixed_std, np.float32), critic_dims=cfg.critic_dims, policy_dims=cfg.policy_dims)
    old, new = OldEntry(**kw), AgentCore(**kw)
    assert list(old.leaves.items()) == list(new.leaves.items()) and np.array_equal(old.fixed_std, new.fixed_std)
    b = AH.synth_batch(cfg, B, seed=5)
    n1, n2 = O.make_noise(cfg, B, seed=8), O.make_noise(cfg, B, seed=9, utd_ratio=2)
    for core in (old, new):
        AH.load_leaves(core, cfg, None, theta)
        core.update_critics(AH.batch_to_device(cfg, b), AH.noise_to_device(cfg, n1))
        core.update_high_utd(AH.batch_to_device(cfg, b), 2, AH.noise_to_device(cfg, n2))
    assert old.step == new.step > 0 and old.read_info() == new.read_info()
    want = _all_bits(types.SimpleNamespace(core=old))
    for key, v in _all_bits(types.SimpleNamespace(core=new)).items():
        assert _bits_equal(v, want[key]), key


def test_checkpoint_roundtrip_and_both_refusals(gpu, tmp_path):
    """tests/test_policy_modes_gpu.py::test_checkpoint_roundtrip_of_a_uniform_agent for a fixed agent: every leaf back and an
    identical next update (the checkpoint carries no fixed_std: the fresh agent is created with it); a uniform and an exp agent's
    state are refused in words, and so is the fixed state by them, the refused agent untouched"""
    from serl_amd.utils.checkpoint import read_checkpoint_tree, restore_checkpoint, save_checkpoint
    S, A, B = 10, 5, 8
    vec = [0.2, 0.3, 1.0, 0.05, 0.7]
    agent = PF.sac_agent(vec, seed=7, B=B, S=S, A=A)
    for i in range(2):
        agent.update_high_utd(_flat_batch(S, A, B, 10 + i), utd_ratio=2)
    save_checkpoint(str(tmp_path / "fixed"), agent, step=agent.state.step)
    tree = read_checkpoint_tree(str(tmp_path / "fixed"))
    assert sorted(tree["params"]["modules_actor"]) == ["Dense_0", "network"]
    assert "fixed_std" not in tree and "fixed_std" not in tree["params"]["modules_actor"]
    fresh = PF.sac_agent(vec, seed=1, B=B, S=S, A=A)
    restore_checkpoint(str(tmp_path / "fixed"), fresh, restore_rng=True)
    assert fresh.state.step == agent.state.step
    want = _all_bits(agent)
    for key, v in _all_bits(fresh).items():
        assert _bits_equal(v, want[key]), key
    nxt = _flat_batch(S, A, B, 20)
    agent.update_high_utd(nxt, utd_ratio=1)
    fresh.update_high_utd(nxt, utd_ratio=1)
    want = _all_bits(agent)
    for key, v in _all_bits(fresh).items():
        assert _bits_equal(v, want[key]), ("after the next update", key)
    others = {"uniform": MW.sac_agent(256, seed=7, B=B, S=S, A=A, policy_kwargs=PM.policy_kwargs("uniform", True)),
              "exp": MW.sac_agent(256, seed=7, B=B, S=S, A=A)}
    for kind, other in others.items():
        other.update_high_utd(_flat_batch(S, A, B, 10), utd_ratio=2)
        save_checkpoint(str(tmp_path / kind), other, step=other.state.step)
        held = "log_stds" if kind == "uniform" else "Dense_1"
        for target, path, pat in ((fresh, kind, rf"the state holds the policy's std leaves \('modules_actor/{held}'\), this agent's head has a fixed std"),
                                  (other, "fixed", r"the state holds no std leaf of the policy .*this agent's head has")):
            before, step_before = _all_bits(target), target.state.step
            with pytest.raises(ValueError, match=pat + r".*nothing was loaded"):
                restore_checkpoint(str(tmp_path / path), target)
            assert target.state.step == step_before
            for key, v in _all_bits(target).items():
                assert _bits_equal(v, before[key]), ("touched by the refused restore", key)


# ---- data parallel -------------------------------------------------------------------------------------------------------------
def _rows(tree, lo, hi):
    return {k: ({c: m[lo:hi] for c, m in v.items()} if isinstance(v, dict) else (v if k == "redq_idx" else v[lo:hi])) for k, v in tree.items()}


def test_two_shards_of_a_batch_equal_the_full_batch(gpu):
    """tests/test_agent_gpu.py::test_dp_split_equals_full_batch on case (a): the gradient a rank all-reduces has no std entry (the
    vector is a constant of every rank's agent), and two ranks' sums are the full batch's"""
    name = "a_state_two_columns_clipped"
    cfg, B, _ = PF.case_config(name)
    _, theta = PF.init_params(cfg, PF.PARAM_SEED)
    b, noise = AH.synth_batch(cfg, B, seed=5), O.make_noise(cfg, B, seed=9, utd_ratio=1)
    _, pc, pa0, pa1 = _spans(cfg)

    def run(rows, shard):
        core = AH.load_leaves(AH.make_core(cfg, rows, agent_seed=7), cfg, None, theta)
        lo = 0 if shard is None else shard * rows
        if shard is not None:
            core.set_shard(lo, B)
        db, dn = AH.batch_to_device(cfg, _rows(b, lo, lo + rows)), AH.noise_to_device(cfg, _rows(noise, lo, lo + rows))
        core.begin_update()
        core.encode(db)
        core.critic_grads(0, rows, B, dn)
        gc, sc = core.debug("g_critic", pc).astype(np.float64), core.debug("scalars", 3).astype(np.float64)
        core.actor_grads(B, dn)
        return gc, sc, core.debug("g_actor", pa1 - pa0).astype(np.float64), core.debug("scalars", 6)[3:6].astype(np.float64)
    full = run(B, None)
    parts = [run(B // 2, r) for r in range(2)]
    for i, what in enumerate(("g_critic", "critic scalars", "g_actor", "actor scalars")):
        err = AH.rel_err(parts[0][i] + parts[1][i], full[i])
        print(f"two shards vs the full batch, {what}: {err:.2e}")
        # (the bound of tests/test_mlp_dropout_gpu.py's twin of this test: float32 sums of 36 + 36 rows against 72, re-associated)
        assert np.abs(full[i]).max() > 0 and err < 1e-5, what
