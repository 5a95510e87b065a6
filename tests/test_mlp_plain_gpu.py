"""GPU: critic and policy MLPs without LayerNorm (serl_agent_create_layer_norm; use_layer_norm=False per network, mlp.py:29-30) under
the whole update chain, on the case table of tests/mlp_plain.py.  The plain rows are plain_row / plain_bwd_row of csrc/heads.hip.

* oracle parity of update_critics and update_high_utd (UTD 1 and the table's) in both schedules of the chain: info scalars, q,
  target_q, next log-prob, every gradient leaf, the state after the step, at the tolerances of tests/test_agent_gpu.py
  (TOL = 1e-4, _compare_state); the fp64 oracle runs of a case are computed once (mlp_plain.oracle_run) and shared;
* the fused chain against the one-launch-per-operation chain bit for bit, and a plain agent's launch count against the LayerNorm
  agent's of the same shape;
* both flags 1 through serl_agent_create_layer_norm against serl_agent_create_shapes bit for bit; the C ABI's refusals and getter;
* the reference's own update code and initial parameters (tests/golden/plain_*.npz);
* the read-only calls, a checkpoint round trip, and the refusals across LayerNorm / plain."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import drq_oracle as O
from oracle import golden_update as G
import agent_helpers as AH
import golden_replay as GR
import init_golden_helpers as IG
import mlp_plain as MP
import mlp_shapes as MS
from test_agent_gpu import TOL, _compare_state
from test_chain_fusion_gpu import _assert_state_bits, _bits_equal, _launches
from test_evaluate_gpu import _same, _state_of
from test_mlp_shapes_gpu import _pair_launches
from test_mlp_widths_gpu import _Figures, _all_bits, _flat_batch, _grads, _info

pytestmark = pytest.mark.gpu
FUSE = pytest.mark.parametrize("fuse", [True, False], ids=["fused", "unfused"])


@pytest.fixture(autouse=True)
def _general_oracle():
    with MP.installed():
        yield


def _core_of(run, fuse):
    """a fresh agent holding the parameters the case's oracle run started from"""
    cfg = run["cfg"]
    trunk, theta = MP.init_params(cfg, run["seed"])
    return AH.load_leaves(AH.make_core(cfg, run["B"], fuse=fuse), cfg, trunk, theta)


# ---- oracle parity -----------------------------------------------------------------------------------------------------------
@FUSE
@pytest.mark.parametrize("case", MP.CASES, ids=MP.IDS)
def test_update_critics_matches_the_oracle(gpu, case, fuse):
    run = MP.oracle_run(case, "critics")
    cfg, B, st, aux = run["cfg"], run["B"], run["state"], run["aux"]
    core = _core_of(run, fuse)
    assert (core.critic_layer_norm, core.policy_layer_norm) == (cfg.critic_layer_norm, cfg.policy_layer_norm)
    for net, ln, n in (("critic", cfg.critic_layer_norm, len(cfg.critic_dims)), ("actor", cfg.policy_layer_norm, len(cfg.policy_dims))):
        assert [k for k in core.leaves if k.startswith(f"{net}/ln")] == ([f"{net}/ln{j}/{p}" for j in range(1, n + 1) for p in ("scale", "bias")] if ln else [])
    core.update_critics(AH.batch_to_device(cfg, run["batch"]), AH.noise_to_device(cfg, run["noise"]))
    fig = _Figures(f"update_critics {case[0]} {'fused' if fuse else 'unfused'}")
    _info(fig, core.read_info(), run["info"], ("critic_loss", "predicted_qs", "target_qs"))
    fig.add("q", AH.rel_err(core.debug("q", cfg.ensemble * B).reshape(cfg.ensemble, B), aux["q"].numpy()))
    fig.add("target_q", AH.rel_err(core.debug("target_q", B), aux["target_q"].numpy()))
    fig.add("next logp", AH.rel_err(core.debug("logp", B), aux["next_logp"].numpy()))
    _grads(fig, cfg, core, aux["grads"], "g_critic")
    fig.check()
    _compare_state(cfg, st, core)
    assert core.step == st.step == 1
    assert core.debug("ctr_nonzero", 1)[0] == 0


_UTD = [(c, 1) for c in MP.CASES] + [(c, c[8]) for c in MP.CASES if c[8] > 1]


@FUSE
@pytest.mark.parametrize("case,utd", _UTD, ids=[f"{c[0]}-utd{u}" for c, u in _UTD])
def test_update_high_utd_matches_the_oracle(gpu, case, utd, fuse):
    run = MP.oracle_run(case, ("high_utd", utd))
    cfg, B, st = run["cfg"], run["B"], run["state"]
    assert B % utd == 0
    core = _core_of(run, fuse)
    core.update_high_utd(AH.batch_to_device(cfg, run["batch"]), utd, AH.noise_to_device(cfg, run["noise"]))
    fig = _Figures(f"update_high_utd({utd}) {case[0]} {'fused' if fuse else 'unfused'}")
    _info(fig, core.read_info(), run["info"], ("critic_loss", "predicted_qs", "target_qs", "actor_loss", "temperature", "entropy", "temperature_loss"))
    _grads(fig, cfg, core, run["aux"]["g_actor"], "g_actor")
    fig.check()
    _compare_state(cfg, st, core, steps=utd + 1)
    assert core.step == st.step == utd + 1
    assert core.debug("ctr_nonzero", 1)[0] == 0


# ---- fused against un-fused chain, launch counts ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [MP.CASES[1], MP.CASES[2], MP.CASES[6]], ids=[MP.IDS[1], MP.IDS[2], MP.IDS[6]])
def test_fused_chain_is_bit_identical_to_the_unfused_chain(gpu, case):
    cfg, B, _, seed = MP.case_config(case)
    fused, unfused = MP.make_pair(cfg, B, seed=seed, fuse=True)[1], MP.make_pair(cfg, B, seed=seed, fuse=False)[1]
    sl, _ = AH.leaf_slices(cfg)
    pc = sl.get("enc/proprio/ln/bias", sl["critic/head/bias"])[1]
    pa0, pa1 = sl.get("enc/proprio/dense/kernel", sl["actor/w1"])[0], sl["actor/logstd/bias"][1]
    n_pair = {}
    for it in range(2):
        b = AH.synth_batch(cfg, B, seed=300 + it)
        noise = O.make_noise(cfg, B, seed=400 + it, utd_ratio=1)
        for name, core in (("fused", fused), ("unfused", unfused)):
            db, dn = AH.batch_to_device(cfg, b), AH.noise_to_device(cfg, noise)
            torch.cuda.synchronize()
            l0 = _launches()
            core.update_critics(db, dn)
            core.update_high_utd(db, 1, dn)
            torch.cuda.synchronize()
            n_pair[name] = _launches() - l0
        for tap, n in (("g_critic", pc), ("g_actor", pa1 - pa0), ("scalars", 8), ("q", cfg.ensemble * B), ("target_q", B), ("logp", B),
                       ("dx", B * (cfg.enc_dim + cfg.A))):
            assert _bits_equal(fused.debug(tap, n), unfused.debug(tap, n)), (case[0], it, tap)
        fi, pi = fused.read_info(), unfused.read_info()
        assert fi == pi, (case[0], it, fi, pi)
        _assert_state_bits(cfg, fused, unfused, (case[0], it))
    print(f"{case[0]}: chain launches per update_critics + update_high_utd: fused {n_pair['fused']}, one-per-operation {n_pair['unfused']}")
    assert n_pair["fused"] < n_pair["unfused"], n_pair
    assert fused.debug("ctr_nonzero", 1)[0] == 0


@pytest.mark.parametrize("kind,cd,pd,ens", [("state", (256, 256), (256, 256), 10), ("frozen1", (320,), (64, 128, 64), 10),
                                            ("small", (64, 320, 256, 64), (64,), 2)], ids=["state", "frozen1", "small"])
@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "unfused"])
def test_a_plain_layer_takes_the_place_of_its_layer_norm_launch(gpu, kind, cd, pd, ens, fuse):
    """update_critics + update_high_utd(1): a plain agent launches as many kernels as the LayerNorm agent of the same shape --
    the plain forward and backward rows stand where the LayerNorm rows stood, and the bias's column sum is a job of the same
    deferred launch"""
    B = 6
    n = {}
    for name, cln, pln in (("layer_norm", True, True), ("plain", False, False), ("critic_plain", False, True), ("policy_plain", True, False)):
        cfg = MP.config(kind, cd, pd, cln, pln, ensemble=ens)
        n[name] = _pair_launches(MP.make_pair(cfg, B, fuse=fuse)[1], cfg, B, 310)
    print(f"{kind} {'fused' if fuse else 'unfused'}: chain launches per update_critics + update_high_utd(1): {n}")
    assert n["plain"] <= n["layer_norm"] and n["critic_plain"] <= n["layer_norm"] and n["policy_plain"] <= n["layer_norm"], n
    assert n["plain"] == n["layer_norm"], n      # one for one


# ---- (1, 1) through the new entry point is the agent of serl_agent_create_shapes -----------------------------------------------
def _via_layer_norm_entry(flags=(1, 1)):
    from serl_amd.agents.core import AgentCore

    class Core(AgentCore):
        def _create(self, cfg):
            cd, pd = (C.c_int32 * len(self.critic_dims))(*self.critic_dims), (C.c_int32 * len(self.policy_dims))(*self.policy_dims)
            return self.L.serl_agent_create_layer_norm(C.byref(cfg), self._std_param, 0 if self.tanh_squash_distribution else 1, *self._acts,
                                                       cd, len(self.critic_dims), pd, len(self.policy_dims), *flags, C.byref(self._h))
    return Core


def test_both_flags_set_is_the_create_shapes_agent_bit_for_bit(gpu):
    cfg = MS.config("frozen1", (320, 64), (64, 128, 64), critic_activation="swish")
    B = 6
    trunk, theta = MS.init_params(cfg, 42)
    old = MS.make_pair(cfg, B)[1]
    kw = dict(encoder_type=cfg.encoder_type, n_cam=cfg.n_cam, H=cfg.H, W=cfg.W, state_dim=cfg.S, act_dim=cfg.A, batch=B, ensemble=cfg.ensemble,
              hidden=cfg.hidden, discount=cfg.discount, tau=cfg.tau, lr=cfg.lr, warmup_steps=cfg.warmup, dropout=cfg.dropout,
              std_min=cfg.std_min, std_max=cfg.std_max, target_entropy=cfg.target_entropy, seed=0,
              temp_warmup_steps=-1 if cfg.temp_warmup is None else cfg.temp_warmup, critic_subsample_size=cfg.subsample,
              backup_entropy=cfg.backup_entropy, optimizers=cfg.opt, critic_activation=cfg.critic_activation,
              policy_activation=cfg.policy_activation, critic_dims=cfg.critic_dims, policy_dims=cfg.policy_dims)
    new = AH.load_leaves(_via_layer_norm_entry()(**kw), cfg, trunk, theta)
    assert list(new.leaves.items()) == list(old.leaves.items())
    assert [int(c.L.serl_agent_mlp_layer_norm(c._h, net)) for c in (new, old) for net in (0, 1)] == [1, 1, 1, 1]
    b = AH.synth_batch(cfg, B, seed=300)
    noise = O.make_noise(cfg, B, seed=400, utd_ratio=2)
    n = {}
    for name, core in (("new", new), ("old", old)):
        db, dn = AH.batch_to_device(cfg, b), AH.noise_to_device(cfg, noise)
        torch.cuda.synchronize()
        l0 = _launches()
        core.update_high_utd(db, 2, dn)
        torch.cuda.synchronize()
        n[name] = _launches() - l0
    assert new.read_info() == old.read_info()
    _assert_state_bits(cfg, new, old, "(1, 1)")
    assert n["new"] == n["old"], n


def test_c_abi_refusals_and_the_getter(gpu):
    from serl_amd import _lib
    from serl_amd._lib_agent import SerlAgentCfg
    SERL_ERR_INVALID = -1      # include/serl_mi355.h
    L = _lib.lib()
    cfg = SerlAgentCfg(0, 0, 0, 0, 10, 4, 8, 10, 256, 256, 8, 64, 0, -1, 0.99, 0.005, 3e-4, 0.1, 1e-5, 5.0, -2.0, 0)
    dims = (C.c_int32 * 2)(64, 128)

    def create(cln, pln):
        h = C.c_void_p()
        rc = int(L.serl_agent_create_layer_norm(C.byref(cfg), 0, 0, 0, 0, dims, 2, dims, 1, cln, pln, C.byref(h)))
        return rc, (L.serl_last_error() or b"").decode(), h
    for cln, pln, what in ((2, 1, "critic_layer_norm 2"), (-1, 0, "critic_layer_norm -1"), (0, 2, "policy_layer_norm 2"), (1, -1, "policy_layer_norm -1")):
        rc, msg, _ = create(cln, pln)
        assert rc == SERL_ERR_INVALID and what in msg, (cln, pln, rc, msg)
    for cln, pln in ((0, 0), (0, 1), (1, 0), (1, 1)):
        rc, msg, h = create(cln, pln)
        assert rc == 0, msg
        assert (int(L.serl_agent_mlp_layer_norm(h, 0)), int(L.serl_agent_mlp_layer_norm(h, 1))) == (cln, pln)
        assert int(L.serl_agent_mlp_layer_norm(h, 2)) == -1 and int(L.serl_agent_mlp_layer_norm(None, 0)) == -1
        name, count, names = C.create_string_buffer(256), C.c_int64(), []
        for i in range(int(L.serl_agent_num_leaves(h))):
            assert int(L.serl_agent_leaf_info(h, i, name, 256, C.byref(count))) == 0
            names.append(name.value.decode())
        assert ("critic/ln1/scale" in names, "critic/ln2/bias" in names, "actor/ln1/scale" in names) == (bool(cln), bool(cln), bool(pln))
        assert "critic/w2" in names and "critic/b2" in names and "actor/b1" in names
        assert int(L.serl_agent_destroy(h)) == 0
    # an agent of an old entry point has its LayerNorm in both
    core = AH.make_pair(O.Config(image_keys=(), S=10, A=4, hidden=192), 8)[1]
    assert int(core.L.serl_agent_mlp_layer_norm(core._h, 0)) == 1 and int(core.L.serl_agent_mlp_layer_norm(core._h, 1)) == 1


# ---- the reference's own code --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MP.UPDATE_GOLDEN)
def test_hip_update_matches_the_reference_golden(gpu, name):
    """tests/test_golden_update_gpu.py::test_hip_update_matches_the_reference_golden on plain_update_<name>.npz (injected noise)"""
    g = MP.load_golden(name)
    cfg = g["cfg"]
    agent = MP.reference_agent(cfg, g["B"])
    assert (agent.core.critic_layer_norm, agent.core.policy_layer_norm) == (cfg.critic_layer_norm, cfg.policy_layer_norm)
    assert agent.core.critic_dims == cfg.critic_dims and agent.core.policy_dims == cfg.policy_dims
    AH.load_leaves(agent.core, cfg, *O.init_params(cfg, g["meta"]["param_seed"]))
    GR.replay(agent, g, label=f"plain_update_{name}")
    assert agent.core.debug("ctr_nonzero", 1)[0] == 0


def test_reference_init_then_one_update_matches_the_reference(gpu):
    """tests/test_init_reference_gpu.py::test_reference_init_then_one_update_matches_the_reference on plain_init_sac_state.npz:
    from the seed only, param_init="reference", the policy without its LayerNorm leaves"""
    npz, cfg, recs, _ = MP.init_golden()
    g = G.unpack(npz)
    g["cfg"] = cfg
    agent = MP.reference_agent(cfg, g["B"], param_init="reference")
    core = agent.core
    assert (core.critic_layer_norm, core.policy_layer_norm) == (True, False) and not any(k.startswith("actor/ln") for k in core.leaves)
    bad = [m for n in sorted(recs) for sec in ("params", "target_params") for m in [IG.mismatch(n, recs[n], core.get(sec, n))] if m]
    assert not bad, bad
    for n in recs:
        for tx in ("critic", "actor", "temperature"):
            assert not core.get(f"opt/{tx}/mu", n).any() and not core.get(f"opt/{tx}/nu", n).any()
    assert [int(v) for v in agent.state.rng] == g["meta"]["rng0"] == [int(v) for v in npz["init_rng"]]
    assert [s["kind"] for s in g["steps"]] == ["high_utd"] and set(recs) == set(O.trainable_param_shapes(cfg))
    GR.replay(agent, g, seed_only=True, label="plain_init_sac_state")


def test_both_flags_true_under_the_switch_make_the_agent_of_the_call_without_it(gpu):
    with_switch = MS.sac_agent((128, 64), (64,), seed=3, mlp_plain=True)
    without = MS.sac_agent((128, 64), (64,), seed=3)
    assert list(with_switch.core.leaves.items()) == list(without.core.leaves.items()) and with_switch.config == without.config
    want = _all_bits(without)
    for key, v in _all_bits(with_switch).items():
        assert _bits_equal(v, want[key]), key


def test_the_switch_alone_serves_one_h_h_without_mlp_shapes(gpu):
    """mlp_plain=True without mlp_shapes at hidden_dims=[128, 128]: the agent mlp_shapes=True makes of the same kwargs, bit for bit
    after an update"""
    import mlp_widths as MW
    S, A, B = 10, 4, 8
    kw = dict(critic_network_kwargs=MP.mlp_kwargs([128, 128], False), policy_network_kwargs=MP.mlp_kwargs([128, 128], True), mlp_plain=True)
    alone = MW.sac_agent(128, seed=5, B=B, S=S, A=A, **kw)
    both = MW.sac_agent(128, seed=5, B=B, S=S, A=A, mlp_shapes=True, **kw)
    assert (alone.core.critic_layer_norm, alone.core.policy_layer_norm) == (False, True)
    assert list(alone.core.leaves.items()) == list(both.core.leaves.items())
    assert not any(k.startswith("critic/ln") for k in alone.core.leaves) and "actor/ln2/bias" in alone.core.leaves
    assert alone.config["critic_use_layer_norm"] is False and alone.config["policy_use_layer_norm"] is True
    batch = _flat_batch(S, A, B, 10)
    for agent in (alone, both):
        agent.update_high_utd(batch, utd_ratio=2)
    want = _all_bits(both)
    for key, v in _all_bits(alone).items():
        assert _bits_equal(v, want[key]), key
    assert np.isfinite(alone.core.get("params", "critic/w1")).all()


# ---- the read-only calls ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [MP.CASES[1], MP.CASES[2], MP.CASES[3]], ids=[MP.IDS[1], MP.IDS[2], MP.IDS[3]])
def test_q_values_and_policy_stats_match_the_oracle(gpu, case):
    cfg, B, _, seed = MP.case_config(case)
    st, core = MP.make_pair(cfg, B, seed=seed)
    b = AH.synth_batch(cfg, B, seed=6)
    state, act = torch.tensor(b["state"], device="cuda"), torch.tensor(b["action"], device="cuda")
    enc = torch.tensor(b["state"], dtype=torch.float64)
    mean, std = O.policy_head(st.params, cfg, enc)
    fig = _Figures(f"read-only {case[0]}")
    for target, th in ((False, st.params), (True, st.target)):
        q = O.critic_forward(th, cfg, enc, torch.tensor(b["action"], dtype=torch.float64))
        fig.add(f"q target={target}", AH.rel_err(core.eval_q(None, state, act, target=target).cpu().numpy(), q.numpy()))
    pol = {k: v.cpu().numpy() for k, v in core.eval_policy(None, state, None).items()}
    fig.add("mean", AH.rel_err(pol["mean"], mean.numpy()))
    fig.add("std", AH.rel_err(pol["std"], std.numpy()))
    fig.add("mode", AH.rel_err(pol["mode"], torch.tanh(mean).numpy()))
    fig.check()
    # sample_actions against the statistics: the mode is the argmax action, and the std that of an update's own policy evaluation
    assert np.array_equal(pol["mode"], core.sample_actions(None, state, None).cpu().numpy())
    db = AH.batch_to_device(cfg, b)
    core.update(db, ("actor",), AH.noise_to_device(cfg, O.make_noise(cfg, B, seed=3)))     # its policy evaluation: obs, old parameters
    assert np.array_equal(pol["std"].reshape(-1), core.debug("std", B * cfg.A))
    assert core.debug("ctr_nonzero", 1)[0] == 0


def test_read_only_calls_leave_a_plain_agent_byte_for_byte(gpu):
    S, A, B = 10, 4, 8
    agent = MP.sac_agent((128, 64), (64, 320), False, False, seed=7, B=B, S=S, A=A)
    agent.update_high_utd(_flat_batch(S, A, B, 10), utd_ratio=2)          # away from step 0 and from zero moments
    torch.cuda.synchronize()
    before = _state_of(agent)
    rng = np.random.default_rng(4)
    state, act = rng.standard_normal((B, S)).astype(np.float32), rng.uniform(-0.9, 0.9, (B, A)).astype(np.float32)
    batch = _flat_batch(S, A, B, 11)
    q, qt = agent.q_values(state, act), agent.q_values(state, act, target=True)
    stats = agent.policy_stats(state, act)
    assert q.shape == qt.shape == (10, B) and np.isfinite(q).all() and np.isfinite(stats["log_prob"]).all()
    assert np.array_equal(stats["mode"], agent.sample_actions(state, argmax=True))
    ev = agent.evaluate_batch(batch, side="next_observations")
    losses = agent.evaluate_losses(batch)
    assert np.isfinite(ev["q"]).all() and losses is not None
    torch.cuda.synchronize()
    assert _same(before, _state_of(agent)) == []


def test_evaluate_losses_equals_the_updates_own_info_on_a_one_layer_plain_critic(gpu):
    cfg, B, _, seed = MP.case_config(MP.CASES[1])
    _, core = MP.make_pair(cfg, B, seed=seed)
    db = AH.batch_to_device(cfg, AH.synth_batch(cfg, B, seed=11))
    noise = O.make_noise(cfg, B, seed=12)
    dry = core.eval_losses(db, AH.noise_to_device(cfg, noise))
    core.update(db, noise=AH.noise_to_device(cfg, noise))
    for k, v in core.read_info().items():
        assert dry[k] == v, (k, dry[k], v)


# ---- checkpoints ---------------------------------------------------------------------------------------------------------------
def test_checkpoint_roundtrip_and_the_refusals_across_layer_norm_and_plain(gpu):
    """a plain-critic agent through agent.snapshot(...) -> restore into a fresh agent -> every leaf back and a bit-identical next
    update; a LayerNorm state into the plain agent and the other way round are refused with an error that says so, the agent untouched"""
    from serl_amd.utils.checkpoint import load_state_dict
    S, A, B = 10, 4, 8
    cd, pd = (128, 64), (64,)
    agent = MP.sac_agent(cd, pd, False, True, seed=7, B=B, S=S, A=A)
    for i in range(2):
        agent.update_high_utd(_flat_batch(S, A, B, 10 + i), utd_ratio=2)
    tree = agent.state.params
    assert sorted(tree["modules_critic"]["network"]) == ["Dense_0", "Dense_1"]
    assert sorted(tree["modules_actor"]["network"]) == ["Dense_0", "LayerNorm_0"]
    snap = agent.snapshot(("params", "target_params", "opt_states"))
    sd = {"params": snap.params, "target_params": snap.target_params, "opt_states": snap.opt_states, "step": snap.step}
    fresh = MP.sac_agent(cd, pd, False, True, seed=1, B=B, S=S, A=A)
    load_state_dict(fresh, sd)
    fresh._rng_key = agent._rng_key.copy()
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
    with_ln = MP.sac_agent(cd, pd, True, True, seed=3, B=B, S=S, A=A)
    for src, dst, pat in ((agent, with_ln, r"the state's critic MLP has no LayerNorm .*this agent's critic MLP has one; nothing was loaded"),
                          (with_ln, agent, r"'modules_critic/network/LayerNorm_0' is a LayerNorm in the state, this agent's critic MLP has none")):
        before, step_before = _all_bits(dst), dst.state.step
        state = {"params": src.state.params, "target_params": src.state.target_params, "opt_states": src.state.opt_states, "step": 5}
        with pytest.raises(ValueError, match=pat):
            load_state_dict(dst, state)
        assert dst.state.step == step_before
        for key, v in _all_bits(dst).items():
            assert _bits_equal(v, before[key]), ("touched by the refused restore", key)
