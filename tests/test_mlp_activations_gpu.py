"""GPU: relu and swish beside tanh in the critic's and the policy's MLP (serl_agent_create_mlp's critic_act / policy_act; the `act`
field of LnFwdArgs / LnBwdArgs in serl_amd/csrc/heads.hip: ln_activate, ln_act_grad).

* the reference's own update code with another activation (tests/golden/act_*.npz, injected noise) through
  tests/golden_replay.py::replay: its comparisons, its TOL;
* the three row layouts (width 64, blocked 256, strided 2..16 columns per lane) against the oracle with the Config's
  activations: swish and relu at hidden 64, 192, 256 and 1024, 8 rows x 10 members, and 72 rows at 192 -- one
  update_critics and one update_high_utd(1) each, every gradient leaf, the info scalars, the state;
* sample_actions of a swish agent, mode and seeded;
* a tanh agent made by serl_agent_create_mlp(.., 0, 0) against one made by serl_agent_create, bit for bit;
* the C ABI's range checks.

ReLU's kink.  A relu comparison counts only where the fp64 side's relu pre-activations all stay KINK_MIN = 1e-4 away from 0 (an
fp32 run could land on the other side and flip a gradient term); the batch seed moves on, ten seeds at the most, and a width where
none qualifies is skipped with the reason.  From O.init_params' LayerNorm leaves that margin is out of reach of every shape here (a
case evaluates 3e4 to 6e5 relu pre-activations of density 0.4 at 0), so the row cases with a relu network start, like the relu
fixtures, from mlp_activations.kink_margin's leaves: ROW_LIVE live columns per LayerNorm vector whose sign changes from row to
row, all others on in every row or off in every row, their scale following the width (mlp_activations.safe_scale).  Every
case then finds its seed among the ten (asserted in tests/test_mlp_activations_cpu.py, which needs no GPU): nothing skips."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import torch

from oracle import drq_oracle as O
import agent_helpers as AH
import golden_replay as GR
import mlp_activations as MA
import mlp_widths as MW
from test_agent_gpu import TOL, _compare_state
from test_mlp_activations_cpu import _need_golden
from test_mlp_widths_gpu import _Figures, _flat_batch, _grads, _info

pytestmark = pytest.mark.gpu


# ---- the reference's own code with another activation ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MA.GOLDEN))
def test_hip_update_matches_the_reference_golden_with_activation(gpu, name):
    _need_golden(name)
    g, meta, _ = GR.load_variant("act", name)
    cfg, B = g["cfg"], g["B"]
    critic, policy = meta["activations"]["critic"], meta["activations"]["policy"]
    assert (critic, policy) == MA.GOLDEN[name][3] and B == MA.GOLDEN[name][1] and cfg == MA.GOLDEN[name][0]
    agent = GR.reference_agent(cfg, B, critic_network_kwargs=MA.network_kwargs(critic, cfg.hidden),
                               policy_network_kwargs=MA.network_kwargs(policy, cfg.hidden))
    assert (agent.config["critic_activation"], agent.config["policy_activation"]) == (critic, policy)
    assert (agent.core.critic_activation, agent.core.policy_activation) == (critic, policy)
    AH.load_leaves(agent.core, cfg, *MA.initial_leaves(name))
    GR.replay(agent, g, label=f"act_{name}")
    assert agent.core.debug("ctr_nonzero", 1)[0] == 0


# ---- the three row layouts against the restated oracle ---------------------------------------------------------------------------
# (id, hidden, rows): 256 = the blocked rows (ln_row<4, true>); 64 / 192 / 1024 = the strided rows at 1, 3 and 16 columns per lane.
# 8 rows = two LayerNorm workgroups per member; 72 rows = two 64-row GEMM tiles, the second ragged.
ROWS = [("w64_B8", 64, 8), ("w192_B8", 192, 8), ("w256_B8", 256, 8), ("w1024_B8", 1024, 8), ("w192_B72", 192, 72)]


ROW_LIVE = {8: 8, 72: 2}      # live columns per LayerNorm vector by rows: about 1e4 live relu pre-activations per case
PAIRS = [("swish", "swish"), ("relu", "relu"), ("relu", "swish"), ("swish", "relu")]      # (critic, policy)


def _row_cfg(hidden, critic="tanh", policy="tanh"):
    return O.Config(image_keys=(), S=10, A=3, discount=0.99, hidden=hidden, ensemble=10, critic_activation=critic, policy_activation=policy)


def _core(cfg, B, theta):
    """AgentCore of the Config (its activations) holding `theta` (oracle names) in params and target_params"""
    return AH.load_leaves(AH.make_core(cfg, B), cfg, None, theta)


@functools.lru_cache(maxsize=None)
def _oracle_side(hidden, B, critic, policy, margin):
    """the fp64 side of a row case, once per case: update_critics on batch 3 + 16 k, then update_high_utd(1) on batch 4 + 16 k, for
    the first k < KINK_SEEDS whose relu pre-activations all stay `margin` away from 0 (k = 0 without a relu network)
    -> (k, what the comparison needs), or (None, [(k, the |pre-activation| that put seed k out) ...])"""
    cfg = _row_cfg(hidden, critic, policy)
    relu = "relu" in (critic, policy)
    tried = []
    trunk, theta = O.init_params(cfg, 42)
    if relu:
        theta = MA.kink_margin(theta, n_live=ROW_LIVE[B])
    for k in range(MA.KINK_SEEDS if relu else 1):
        st = O.TrainState(cfg, trunk, theta, torch.float64)
        b1, b2 = AH.synth_batch(cfg, B, seed=3 + 16 * k), AH.synth_batch(cfg, B, seed=4 + 16 * k)
        n1, n2 = O.make_noise(cfg, B, seed=7), O.make_noise(cfg, B, seed=8, utd_ratio=1)
        recs = {w: MA.Recorder(floor=margin if a == "relu" else None) for w, a in (("critic", critic), ("policy", policy))}
        try:
            with O.observe_preactivations(recs):
                info1, aux1 = O.update_critics(st, AH.batch_to_torch(b1, torch.float64), O.noise_to_torch(n1, torch.float64))
                info2, aux2 = O.update_high_utd(st, AH.batch_to_torch(b2, torch.float64), O.noise_to_torch(n2, torch.float64), 1)
        except MA.Kink as e:      # this seed is out at its first evaluation inside the margin
            tried.append((k, e.args[0]))
            continue
        return k, dict(theta=theta, b1=b1, b2=b2, n1=n1, n2=n2, info1=info1, aux1=aux1, info2=info2, aux2=aux2, st=st, recs=recs)
    return None, tried


def _compare_rows(case, critic, policy, margin):
    label, hidden, B = case
    cfg = _row_cfg(hidden, critic, policy)
    k, side = _oracle_side(hidden, B, critic, policy, margin)
    if k is None:
        pytest.skip(f"{label} {critic}/{policy}: no batch seed among {MA.KINK_SEEDS} keeps every relu pre-activation {margin:g} away from 0 "
                    f"(seed index, the first evaluation's minimum inside the margin): {[(i, float(f'{m:.2g}')) for i, m in side]}")
    core = _core(cfg, B, side["theta"])
    assert core.cfg.hidden == hidden and (core.critic_activation, core.policy_activation) == (critic, policy)
    fig = _Figures(f"{label} critic={critic} policy={policy} seed {k}")
    core.update_critics(AH.batch_to_device(cfg, side["b1"]), AH.noise_to_device(cfg, side["n1"]))
    _info(fig, core.read_info(), side["info1"], ("critic_loss", "predicted_qs", "target_qs"))
    fig.add("q", AH.rel_err(core.debug("q", cfg.ensemble * B).reshape(cfg.ensemble, B), side["aux1"]["q"].numpy()))
    fig.add("target_q", AH.rel_err(core.debug("target_q", B), side["aux1"]["target_q"].numpy()))
    fig.add("next logp", AH.rel_err(core.debug("logp", B), side["aux1"]["next_logp"].numpy()))
    _grads(fig, cfg, core, side["aux1"]["grads"], "g_critic")
    core.update_high_utd(AH.batch_to_device(cfg, side["b2"]), 1, AH.noise_to_device(cfg, side["n2"]))
    _info(fig, core.read_info(), side["info2"],
          ("critic_loss", "predicted_qs", "target_qs", "actor_loss", "temperature", "entropy", "temperature_loss"))
    _grads(fig, cfg, core, side["aux2"]["g_actor"], "g_actor")
    fig.check()
    _compare_state(cfg, side["st"], core, steps=3)
    assert core.step == side["st"].step == 3
    assert core.debug("ctr_nonzero", 1)[0] == 0


@pytest.mark.parametrize("critic,policy", PAIRS, ids=["swish", "relu", "relu_swish", "swish_relu"])
@pytest.mark.parametrize("case", ROWS, ids=[r[0] for r in ROWS])
def test_rows_match_the_restated_oracle(gpu, case, critic, policy):
    """swish and relu in both networks, and the two mixed pairs: the critic's and the policy's code are independent"""
    _compare_rows(case, critic, policy, MA.KINK_MIN)


def test_a_tanh_row_case_fails_against_the_swish_oracle(gpu):
    """the comparison above can tell the activations apart: a tanh agent is far from the swish oracle"""
    label, hidden, B = ROWS[0]
    cfg = _row_cfg(hidden)
    _, side = _oracle_side(hidden, B, "swish", "swish", MA.KINK_MIN)
    core = _core(cfg, B, side["theta"])
    core.update_critics(AH.batch_to_device(cfg, side["b1"]), AH.noise_to_device(cfg, side["n1"]))
    assert AH.rel_err(core.debug("q", cfg.ensemble * B).reshape(cfg.ensemble, B), side["aux1"]["q"].numpy()) > 100 * TOL


# ---- sample_actions --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", [256, 192], ids=["w256", "w192"])
def test_sample_actions_of_a_swish_agent_match_the_restated_policy(gpu, hidden):
    S, A, B = 10, 5, 72
    agent = MW.sac_agent(hidden, seed=3, B=B, S=S, A=A, critic_network_kwargs=MA.network_kwargs("relu", hidden),
                         policy_network_kwargs=MA.network_kwargs("swish", hidden))
    cfg = O.Config(image_keys=(), S=S, A=A, discount=0.99, hidden=hidden, critic_activation="relu", policy_activation="swish")
    theta = MA.act_theta(O.init_params(cfg, GR.PARAM_SEED)[1], cfg, "trained")      # (LayerNorm scales up to 3: swish is not near-linear)
    AH.load_leaves(agent.core, cfg, None, theta)
    state = np.random.default_rng(6).standard_normal((B, S)).astype(np.float32)
    th = O.to_torch(theta, torch.float64)
    mean, sd = O.policy_head(th, cfg, torch.tensor(state, dtype=torch.float64))
    mode = agent.sample_actions(state, argmax=True)
    e_mode = AH.rel_err(mode, torch.tanh(mean).numpy())
    seed = np.array([0, 11], np.uint32)
    got = agent.sample_actions(state, seed=seed)
    eps = agent._action_noise(seed, B).cpu().numpy().astype(np.float64)        # the draws that seed stands for
    want, _ = O.sample_and_log_prob(mean, sd, torch.tensor(eps))
    e_sample = AH.rel_err(got, want.numpy())
    tanh_mean, _ = O.policy_head(th, dataclasses.replace(cfg, policy_activation="tanh"), torch.tensor(state, dtype=torch.float64))
    print(f"sample_actions swish w{hidden}: mode {e_mode:.2e}, sample {e_sample:.2e}; "
          f"the tanh policy's mode is {AH.rel_err(torch.tanh(tanh_mean).numpy(), torch.tanh(mean).numpy()):.2e} away")
    assert e_mode < TOL and e_sample < TOL
    assert AH.rel_err(torch.tanh(tanh_mean).numpy(), torch.tanh(mean).numpy()) > 100 * TOL
    assert not np.array_equal(got, mode) and np.array_equal(got, agent.sample_actions(state, seed=seed))


# ---- the default agent is the one it was -----------------------------------------------------------------------------------------
def _bits(core):
    return {(sec, leaf): core.get(sec, leaf).copy() for leaf in core.leaves
            for sec in ("params", "target_params", "opt/critic/mu", "opt/critic/nu", "opt/actor/mu", "opt/actor/nu",
                        "opt/temperature/mu", "opt/temperature/nu")}


@pytest.mark.parametrize("hidden", [256, 64, 192], ids=["w256", "w64", "w192"])
def test_tanh_through_create_mlp_is_bit_identical_to_serl_agent_create(gpu, hidden):
    from serl_amd.agents.core import AgentCore

    class OldEntry(AgentCore):
        def _create(self, cfg):
            return self.L.serl_agent_create(C.byref(cfg), C.byref(self._h))

    cfg, B = _row_cfg(hidden), 72
    _, theta = O.init_params(cfg, 42)
    kw = dict(encoder_type=cfg.encoder_type, n_cam=0, H=0, W=0, state_dim=cfg.S, act_dim=cfg.A, batch=B, ensemble=cfg.ensemble,
              hidden=hidden, discount=cfg.discount, tau=cfg.tau, lr=cfg.lr, warmup_steps=cfg.warmup, dropout=cfg.dropout,
              std_min=cfg.std_min, std_max=cfg.std_max, target_entropy=cfg.target_entropy, seed=0, temp_warmup_steps=-1)
    old, new = OldEntry(**kw), AgentCore(critic_activation="tanh", policy_activation="tanh", **kw)
    assert new._acts == (0, 0)
    b, noise = AH.synth_batch(cfg, B, seed=5), O.make_noise(cfg, B, seed=9, utd_ratio=2)
    for core in (old, new):
        AH.load_leaves(core, cfg, None, theta)
        core.update_high_utd(AH.batch_to_device(cfg, b), 2, AH.noise_to_device(cfg, noise))
    assert old.step == new.step == 3 and old.read_info() == new.read_info()
    want = _bits(old)
    assert any(v.any() for (sec, _), v in want.items() if sec.startswith("opt/actor"))
    for key, v in _bits(new).items():
        assert np.array_equal(v.view(np.uint32), want[key].view(np.uint32)), key


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def _create_mlp(critic_act, policy_act):
    from serl_amd import _lib
    from serl_amd._lib_agent import SerlAgentCfg
    L = _lib.lib()
    cfg = SerlAgentCfg(0, 0, 0, 0, 10, 4, 8, 10, 256, 256, 8, 64, 0, -1, 0.99, 0.005, 3e-4, 0.1, 1e-5, 5.0, -2.0, 0)
    h = C.c_void_p()
    rc = int(L.serl_agent_create_mlp(C.byref(cfg), 0, 0, critic_act, policy_act, C.byref(h)))
    msg = (L.serl_last_error() or b"").decode()
    names = []
    if rc == 0:
        buf, cnt = C.create_string_buffer(128), C.c_int64()
        for i in range(L.serl_agent_num_leaves(h)):
            assert L.serl_agent_leaf_info(h, i, buf, 128, C.byref(cnt)) == 0
            names.append(buf.value.decode())
        assert int(L.serl_agent_destroy(h)) == 0
    return rc, msg, names


def test_c_abi_activation_codes(gpu):
    SERL_ERR_INVALID = -1      # include/serl_mi355.h
    before = list(O.trainable_param_shapes(O.Config(image_keys=(), S=10, A=4)))
    for critic_act in (0, 1, 2):
        for policy_act in (0, 1, 2):
            rc, msg, names = _create_mlp(critic_act, policy_act)
            assert rc == 0 and names == before, (critic_act, policy_act, rc, msg)      # an activation owns no leaf
    for bad, which in (((3, 0), "critic_act 3"), ((0, -1), "policy_act -1"), ((7, 7), "critic_act 7")):
        rc, msg, _ = _create_mlp(*bad)
        assert rc == SERL_ERR_INVALID and which in msg, (bad, rc, msg)
        assert "SERL_ACT_TANH (0), SERL_ACT_RELU (1) and SERL_ACT_SWISH (2)" in msg, msg


def test_checkpoint_holds_no_activation_and_restores_across_them(gpu, tmp_path):
    """the flax checkpoint is agent.state alone (params, target_params, opt_states, step, rng): an activation owns no leaf, so the
    file of a swish agent restores into a swish agent bit for bit (and the next update is identical) -- and ALSO loads into a tanh
    agent of the same geometry without complaint, which then computes something else: the gap INTEGRATION.md documents; the caller
    constructs the agent with the kwargs of the run"""
    from serl_amd.utils.checkpoint import read_checkpoint_tree, restore_checkpoint, save_checkpoint
    S, A, B = 10, 4, 8
    nk = dict(critic_network_kwargs=MA.network_kwargs("swish", 128), policy_network_kwargs=MA.network_kwargs("swish", 128))
    agent = MW.sac_agent(128, seed=7, B=B, S=S, A=A, **nk)
    agent.update_high_utd(_flat_batch(S, A, B, 10), utd_ratio=2)
    save_checkpoint(str(tmp_path / "swish"), agent, step=agent.state.step)
    assert set(read_checkpoint_tree(str(tmp_path / "swish"))) == {"step", "params", "target_params", "opt_states", "rng"}
    fresh = MW.sac_agent(128, seed=1, B=B, S=S, A=A, **nk)
    other = MW.sac_agent(128, seed=1, B=B, S=S, A=A)      # the launcher's tanh
    assert other.config["critic_activation"] == "tanh" and fresh.config["critic_activation"] == "swish"
    want = _bits(agent.core)
    for target in (fresh, other):
        restore_checkpoint(str(tmp_path / "swish"), target, restore_rng=True)
        assert target.state.step == agent.state.step
        for key, v in _bits(target.core).items():
            assert np.array_equal(v.view(np.uint32), want[key].view(np.uint32)), key
    nxt = _flat_batch(S, A, B, 20)
    for a in (agent, fresh, other):
        a.update_high_utd(nxt, utd_ratio=1)
    want = _bits(agent.core)
    for key, v in _bits(fresh.core).items():
        assert np.array_equal(v.view(np.uint32), want[key].view(np.uint32)), ("after the next update", key)
    got = _bits(other.core)      # the same state under tanh MLPs: another update
    assert not np.array_equal(got[("params", "critic/w1")], want[("params", "critic/w1")])
