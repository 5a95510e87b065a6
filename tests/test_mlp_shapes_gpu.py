"""GPU: critic and policy MLPs of their own depth and per-layer widths (serl_agent_create_shapes; hidden_dims of 1 to 4 layers per
network, every width a multiple of 64 in [64, 1024]) under the whole update chain, on the case table of tests/mlp_shapes.py.

* oracle parity of update_critics, update_high_utd (UTD 1 and the table's) and sample_actions: info scalars, q, target_q, next
  log-prob, every gradient leaf, the state after the step, at the tolerances of tests/test_agent_gpu.py (TOL = 1e-4, _compare_state);
* serl_agent_create_shapes({192, 192}, {192, 192}) against serl_agent_create_mlp at hidden = 192: leaf tables, bits, launch count;
* the fused chain against the one-launch-per-operation chain bit for bit, and the launch counts;
* the reference's own update code and initial parameters (tests/golden/shapes_*.npz);
* data-parallel split, checkpoints, the C ABI's refusals, evaluate_losses."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import drq_oracle as O
from oracle import golden_update as G
import agent_helpers as AH
import golden_replay as GR
import init_golden_helpers as IG
import mlp_shapes as MS
from test_agent_gpu import TOL, _compare_state
from test_chain_fusion_gpu import _assert_state_bits, _bits_equal, _launches
from test_mlp_widths_gpu import _Figures, _all_bits, _flat_batch, _grads, _info

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _general_oracle():
    with MS.installed():
        yield


# ---- oracle parity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MS.CASES, ids=MS.IDS)
def test_update_critics_matches_the_oracle(gpu, case):
    cfg, B, _ = MS.case_config(case)
    st, core = MS.make_pair(cfg, B)
    assert core.critic_dims == cfg.critic_dims and core.policy_dims == cfg.policy_dims
    assert core.leaves[f"actor/w{len(cfg.policy_dims)}"] == ([cfg.enc_dim] + list(cfg.policy_dims))[-2] * cfg.policy_dims[-1]
    b = AH.synth_batch(cfg, B, seed=3)
    noise = O.make_noise(cfg, B, seed=7)
    info, aux = O.update_critics(st, AH.batch_to_torch(b, torch.float64), O.noise_to_torch(noise, torch.float64))
    core.update_critics(AH.batch_to_device(cfg, b), AH.noise_to_device(cfg, noise))
    fig = _Figures(f"update_critics {case[0]}")
    _info(fig, core.read_info(), info, ("critic_loss", "predicted_qs", "target_qs"))
    fig.add("q", AH.rel_err(core.debug("q", cfg.ensemble * B).reshape(cfg.ensemble, B), aux["q"].numpy()))
    fig.add("target_q", AH.rel_err(core.debug("target_q", B), aux["target_q"].numpy()))
    fig.add("next logp", AH.rel_err(core.debug("logp", B), aux["next_logp"].numpy()))
    _grads(fig, cfg, core, aux["grads"], "g_critic")
    fig.check()
    _compare_state(cfg, st, core)
    assert core.step == st.step == 1
    assert core.debug("ctr_nonzero", 1)[0] == 0


_UTD = [(c, 1) for c in MS.CASES] + [(c, u) for c in MS.CASES for u in ((c[6],) if c[6] > 1 else ()) + MS.EXTRA_UTD.get(c[0], ())]


@pytest.mark.parametrize("case,utd", _UTD, ids=[f"{c[0]}-utd{u}" for c, u in _UTD])
def test_update_high_utd_matches_the_oracle(gpu, case, utd):
    cfg, B, _ = MS.case_config(case)
    assert B % utd == 0
    st, core = MS.make_pair(cfg, B)
    b = AH.synth_batch(cfg, B, seed=4)
    noise = O.make_noise(cfg, B, seed=8, utd_ratio=utd)
    info, aux = O.update_high_utd(st, AH.batch_to_torch(b, torch.float64), O.noise_to_torch(noise, torch.float64), utd)
    core.update_high_utd(AH.batch_to_device(cfg, b), utd, AH.noise_to_device(cfg, noise))
    fig = _Figures(f"update_high_utd({utd}) {case[0]}")
    _info(fig, core.read_info(), info, ("critic_loss", "predicted_qs", "target_qs", "actor_loss", "temperature", "entropy", "temperature_loss"))
    _grads(fig, cfg, core, aux["g_actor"], "g_actor")
    fig.check()
    _compare_state(cfg, st, core, steps=utd + 1)
    assert core.step == st.step == utd + 1
    assert core.debug("ctr_nonzero", 1)[0] == 0


@pytest.mark.parametrize("case", MS.CASES, ids=MS.IDS)
def test_sample_actions_match_the_oracle(gpu, case):
    cfg, B, _ = MS.case_config(case)
    st, core = MS.make_pair(cfg, B)
    b = AH.synth_batch(cfg, B, seed=6)
    frames = torch.tensor(np.stack([b["obs"][k] for k in cfg.image_keys]), device="cuda") if cfg.image_keys else None
    state = torch.tensor(b["state"], device="cuda")
    feats = O.features(st, {k: torch.tensor(v) for k, v in b["obs"].items()})
    enc = O.encode(st.params, cfg, feats, torch.tensor(b["state"], dtype=torch.float64))
    mean, std = O.policy_head(st.params, cfg, enc)
    fig = _Figures(f"sample_actions {case[0]}")
    fig.add("mode", AH.rel_err(core.sample_actions(frames, state, None).cpu().numpy(), torch.tanh(mean).numpy()))
    eps = np.random.default_rng(0).standard_normal((B, cfg.A)).astype(np.float32)
    a, _ = O.sample_and_log_prob(mean, std, torch.tensor(eps, dtype=torch.float64))
    fig.add("sample", AH.rel_err(core.sample_actions(frames, state, torch.tensor(eps, device="cuda")).cpu().numpy(), a.numpy()))
    fig.check()
    assert core.debug("ctr_nonzero", 1)[0] == 0


def test_debug_taps_exist_for_every_layer(gpu):
    cfg, B, _ = MS.case_config(MS.CASES[2])
    st, core = MS.make_pair(cfg, B)
    core.update_high_utd(AH.batch_to_device(cfg, AH.synth_batch(cfg, B, seed=4)), 1, AH.noise_to_device(cfg, O.make_noise(cfg, B, seed=8)))
    for l, w in enumerate(cfg.critic_dims, 1):
        assert np.isfinite(core.debug(f"mlp_xhat/crit_/{l}", cfg.ensemble * B * w)).all()
        assert np.isfinite(core.debug(f"mlp_dpre/{l}", B * w)).all()
    for l, w in enumerate(cfg.policy_dims, 1):
        x = core.debug(f"mlp_xhat/pol__/{l}", B * w).reshape(B, w)
        assert np.abs(x.mean(1)).max() < 1e-4 and np.abs(x.var(1) - 1).max() < 1e-2       # a LayerNorm's normalised rows
    from serl_amd import _lib
    with pytest.raises(_lib.SerlError):
        core.debug(f"mlp_xhat/pol__/{len(cfg.policy_dims) + 1}", 1)


# ---- [h, h] through the new entry point is the agent of the old one ---------------------------------------------------------------
def test_shapes_entry_point_at_h_h_is_the_create_mlp_agent(gpu):
    cfg = MS.config("frozen1", (192, 192), (192, 192))
    old_cfg = O.Config(image_keys=("wrist",), H=64, W=64, S=5, A=3, hidden=192)
    B = 6
    new, old = MS.make_pair(cfg, B)[1], AH.make_pair(old_cfg, B)[1]
    # (the new core sends its two lists, the old one n_layers = 0: two layers of cfg.hidden)
    assert (new.spec.to_c().critic.n_layers, new.spec.to_c().policy.n_layers) == (2, 2)
    assert (old.spec.to_c().critic.n_layers, old.spec.to_c().policy.n_layers) == (0, 0) and old.critic_dims == old.policy_dims == (192, 192)
    assert list(new.leaves.items()) == list(old.leaves.items())
    n = {}
    for it in range(2):
        b = AH.synth_batch(cfg, B, seed=300 + it)
        noise = O.make_noise(cfg, B, seed=400 + it, utd_ratio=2)
        for name, core in (("new", new), ("old", old)):
            db, dn = AH.batch_to_device(cfg, b), AH.noise_to_device(cfg, noise)
            torch.cuda.synchronize()
            l0 = _launches()
            core.update_high_utd(db, 2, dn)
            torch.cuda.synchronize()
            n[name] = _launches() - l0
        assert new.read_info() == old.read_info()
        _assert_state_bits(cfg, new, old, ("[h, h]", it))
    assert n["new"] == n["old"], n


# ---- fused against un-fused chain ----------------------------------------------------------------------------------------------
def _pair_launches(core, cfg, B, seed):
    """chain launches of one update_critics + one update_high_utd(1)"""
    db, dn = AH.batch_to_device(cfg, AH.synth_batch(cfg, B, seed=seed)), AH.noise_to_device(cfg, O.make_noise(cfg, B, seed=seed + 100, utd_ratio=1))
    torch.cuda.synchronize()
    l0 = _launches()
    core.update_critics(db, dn)
    core.update_high_utd(db, 1, dn)
    torch.cuda.synchronize()
    return _launches() - l0


@pytest.mark.parametrize("case", [MS.CASES[2], MS.CASES[4]], ids=[MS.IDS[2], MS.IDS[4]])
def test_fused_chain_is_bit_identical_to_the_unfused_chain(gpu, case):
    cfg, B, _ = MS.case_config(case)
    fused, plain = MS.make_pair(cfg, B, fuse=True)[1], MS.make_pair(cfg, B, fuse=False)[1]
    sl, _ = AH.leaf_slices(cfg)
    pc = sl.get("enc/proprio/ln/bias", sl["critic/head/bias"])[1]
    pa0, pa1 = sl.get("enc/proprio/dense/kernel", sl["actor/w1"])[0], sl["actor/logstd/bias"][1]
    n_pair = {}
    for it in range(2):
        b = AH.synth_batch(cfg, B, seed=300 + it)
        noise = O.make_noise(cfg, B, seed=400 + it, utd_ratio=1)
        for name, core in (("fused", fused), ("plain", plain)):
            db, dn = AH.batch_to_device(cfg, b), AH.noise_to_device(cfg, noise)
            torch.cuda.synchronize()
            l0 = _launches()
            core.update_critics(db, dn)
            core.update_high_utd(db, 1, dn)
            torch.cuda.synchronize()
            n_pair[name] = _launches() - l0
        for tap, n in (("g_critic", pc), ("g_actor", pa1 - pa0), ("scalars", 8), ("q", cfg.ensemble * B), ("target_q", B), ("logp", B),
                       ("dx", B * (cfg.enc_dim + cfg.A))):
            assert _bits_equal(fused.debug(tap, n), plain.debug(tap, n)), (case[0], it, tap)
        fi, pi = fused.read_info(), plain.read_info()
        assert fi == pi, (case[0], it, fi, pi)
        _assert_state_bits(cfg, fused, plain, (case[0], it))
    print(f"{case[0]}: chain launches per update_critics + update_high_utd: fused {n_pair['fused']}, one-per-operation {n_pair['plain']}")
    assert n_pair["fused"] < n_pair["plain"], n_pair
    assert fused.debug("ctr_nonzero", 1)[0] == 0


def test_added_layers_cost_their_own_launches_and_no_more(gpu):
    """Case 6 (two cameras, four layers of 64 in both MLPs) against the same agent with [64, 64] twice, fused chain, one
    update_critics + one update_high_utd(1) = two critic phases and one actor phase (csrc/agent.hip).  Per added layer:

    * critic phase: the policy at next_obs runs one GEMM and one LayerNorm launch per policy layer (policy_mlp_multi), the target and
      online critics share one GEMM and one LayerNorm launch per critic layer (critic_fwd_multi), and critic_bwd runs one LayerNorm
      backward and one input-gradient GEMM per critic layer: 2 per policy layer, 4 per critic layer.  The layer's column sums and
      weight gradient are jobs of the phase's two deferred launches -- no launch of their own -- until the weight-gradient table
      (kMaxGemmGroups = 6) is full: head + 4 critic layers + proprio fill it, and the camera heads' weight gradient is launched
      on its own (wgrad): 1 more, once per critic phase, with four critic layers.
    * actor phase: both policy evaluations share a layer's two forward launches, the critic adds two forward and two backward
      launches per layer, the policy two backward launches: 4 per policy layer, 4 per critic layer.  Its deferred tables hold
      2 log-prob sums + head bias + 4 layers + proprio = 8 column sums and head + 4 + proprio = 6 weight gradients: they fit.

    Two added layers in each network: 2 x (2 * 2 + 4 * 2 + 1) + (4 * 2 + 4 * 2) = 26 + 16 = 42."""
    cfg6, B, _ = MS.case_config(MS.CASES[5])
    cfg2 = MS.config("frozen2", (64, 64), (64, 64))
    n6 = _pair_launches(MS.make_pair(cfg6, B, fuse=True)[1], cfg6, B, 310)
    n2 = _pair_launches(MS.make_pair(cfg2, B, fuse=True)[1], cfg2, B, 310)
    print(f"fused chain launches per update_critics + update_high_utd(1): 4 + 4 layers {n6}, 2 + 2 layers {n2}")
    assert n6 - n2 == 2 * (2 * 2 + 4 * 2 + 1) + (4 * 2 + 4 * 2), (n6, n2)


# ---- data-parallel split, checkpoints, the C ABI, evaluate_losses ------------------------------------------------------------
def test_dp_split_equals_full_batch_on_four_layers(gpu):
    cfg, B, _ = MS.case_config(MS.CASES[2])
    _, core = MS.make_pair(cfg, B)
    b = AH.synth_batch(cfg, B, seed=5)
    noise = AH.noise_to_device(cfg, O.make_noise(cfg, B, seed=9))
    db = AH.batch_to_device(cfg, b)
    sl, _ = AH.leaf_slices(cfg)
    n = sl["enc/proprio/ln/bias"][1]
    assert core.grad_view(1).numel() >= n
    core.begin_update()
    core.encode(db)
    core.critic_grads(0, B, B, noise)
    full = core.debug("g_critic", n).astype(np.float64)
    sc_full = core.debug("scalars", 3).astype(np.float64)
    parts, scs = [], []
    for r in range(2):
        core.critic_grads(r * (B // 2), B // 2, B, noise)
        parts.append(core.debug("g_critic", n).astype(np.float64))
        scs.append(core.debug("scalars", 3).astype(np.float64))
    assert AH.rel_err(parts[0] + parts[1], full) < 1e-5
    assert AH.rel_err(scs[0] + scs[1], sc_full) < 1e-5


def test_checkpoint_roundtrip_through_a_snapshot(gpu, tmp_path):
    """case 1's shapes through agent.snapshot(("params", "target_params", "opt_states")) -> restore into a fresh agent -> every
    leaf back and a bit-identical next update; a [128, 256]-critic state into a [128, 256, 64]-critic agent and the other way
    round are refused, the agent untouched"""
    from serl_amd.utils.checkpoint import load_state_dict
    S, A, B = 10, 4, 8
    cd, pd = (128, 256), (64,)
    agent = MS.sac_agent(cd, pd, seed=7, B=B, S=S, A=A)
    assert agent.core.critic_dims == cd and agent.core.policy_dims == pd
    for i in range(2):
        agent.update_high_utd(_flat_batch(S, A, B, 10 + i), utd_ratio=2)
    snap = agent.snapshot(("params", "target_params", "opt_states"))
    sd = {"params": snap.params, "target_params": snap.target_params, "opt_states": snap.opt_states, "step": snap.step}
    deep = MS.sac_agent((128, 256, 64), (64, 64, 128), seed=7, B=B, S=S, A=A)
    tree = deep.state.params
    assert tree["modules_critic"]["network"]["Dense_2"]["kernel"].shape == (10, 256, 64)
    assert tree["modules_critic"]["network"]["LayerNorm_2"]["scale"].shape == (10, 64)
    assert tree["modules_actor"]["network"]["Dense_2"]["kernel"].shape == (64, 128)
    assert tree["modules_actor"]["Dense_0"]["kernel"].shape == (128, A)
    fresh = MS.sac_agent(cd, pd, seed=1, B=B, S=S, A=A)
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
    # another depth, both ways: policy lists equal, so that only the critic's depth differs
    two, three = MS.sac_agent((128, 256), (64,), seed=3, B=B, S=S, A=A), MS.sac_agent((128, 256, 64), (64,), seed=3, B=B, S=S, A=A)
    for src, dst, pat in ((two, three, r"leaf 'critic/w3' has \d+ elements in this agent, the state holds 0 "),
                          (three, two, r"'modules_critic/network/Dense_2' holds \d+ elements in the state, this agent's critic MLP has 2 layers")):
        before, step_before = _all_bits(dst), dst.state.step
        state = {"params": src.state.params, "target_params": src.state.target_params, "opt_states": src.state.opt_states, "step": 5}
        with pytest.raises(ValueError, match=pat):
            load_state_dict(dst, state)
        assert dst.state.step == step_before
        for key, v in _all_bits(dst).items():
            assert _bits_equal(v, before[key]), ("touched by the refused restore", key)


def _create_shapes(critic, policy, hidden=256):
    """serl_agent_create_shapes with a state-only configuration -> (status, serl_last_error(), the dims read back)"""
    from serl_amd import _lib
    from serl_amd._lib_agent import SerlAgentCfg
    L = _lib.lib()
    cfg = SerlAgentCfg(0, 0, 0, 0, 10, 4, 8, 10, hidden, 256, 8, 64, 0, -1, 0.99, 0.005, 3e-4, 0.1, 1e-5, 5.0, -2.0, 0)
    h = C.c_void_p()
    arr = lambda v: None if v is None else (C.c_int32 * max(len(v[0]), 1))(*v[0])  # noqa: E731
    rc = int(L.serl_agent_create_shapes(C.byref(cfg), 0, 0, 0, 0, arr(critic), 0 if critic is None else critic[1], arr(policy),
                                        0 if policy is None else policy[1], C.byref(h)))
    msg = (L.serl_last_error() or b"").decode()
    dims = None
    if rc == 0:
        out = (C.c_int32 * 4)()
        dims = tuple(tuple(out[:int(L.serl_agent_mlp_dims(h, net, out))]) for net in (0, 1))
        assert int(L.serl_agent_mlp_dims(h, 2, out)) == -1 and int(L.serl_agent_mlp_dims(None, 0, out)) == -1
        assert int(L.serl_agent_destroy(h)) == 0
    return rc, msg, dims


def test_c_abi_refusals_and_mlp_dims(gpu):
    SERL_ERR_INVALID = -1      # include/serl_mi355.h
    ok = ([64, 64], 2)
    for n in (0, 5):
        rc, msg, _ = _create_shapes(([64] * 5, n), ok)
        assert rc == SERL_ERR_INVALID and f"critic MLP: {n} hidden layers" in msg, (n, rc, msg)
        rc, msg, _ = _create_shapes(ok, ([64] * 5, n))
        assert rc == SERL_ERR_INVALID and f"policy MLP: {n} hidden layers" in msg, (n, rc, msg)
    for w in (0, 100, 1088):
        rc, msg, _ = _create_shapes(([128, w, 64], 3), ok)
        assert rc == SERL_ERR_INVALID and f"critic MLP: layer 2 has width {w}" in msg, (w, rc, msg)
        rc, msg, _ = _create_shapes(ok, ([w], 1))
        assert rc == SERL_ERR_INVALID and f"policy MLP: layer 1 has width {w}" in msg, (w, rc, msg)
    rc, msg, _ = _create_shapes(None, ok)
    assert rc == SERL_ERR_INVALID and "critic_dims is NULL" in msg, (rc, msg)
    rc, msg, _ = _create_shapes(ok, None)
    assert rc == SERL_ERR_INVALID and "policy_dims is NULL" in msg, (rc, msg)
    # cfg->hidden is not read: a value the other entry points refuse
    rc, msg, dims = _create_shapes(([128, 256, 64], 3), ([192], 1), hidden=100)
    assert rc == 0 and dims == ((128, 256, 64), (192,)), (rc, msg, dims)
    rc, msg, dims = _create_shapes(([1024, 64, 64, 1024], 4), ([64, 1024, 64, 64], 4))
    assert rc == 0 and dims == ((1024, 64, 64, 1024), (64, 1024, 64, 64)), (rc, msg, dims)
    # an agent of an old entry point reads {hidden, hidden}
    st, core = AH.make_pair(O.Config(image_keys=(), S=10, A=4, hidden=192), 8)
    out = (C.c_int32 * 4)()
    assert int(core.L.serl_agent_mlp_dims(core._h, 0, out)) == 2 and tuple(out[:2]) == (192, 192)
    assert int(core.L.serl_agent_mlp_dims(core._h, 1, out)) == 2 and tuple(out[:2]) == (192, 192)


def test_evaluate_losses_equals_the_updates_own_info_on_a_one_layer_critic(gpu):
    cfg, B, _ = MS.case_config(MS.CASES[1])
    _, core = MS.make_pair(cfg, B)
    db = AH.batch_to_device(cfg, AH.synth_batch(cfg, B, seed=11))
    noise = O.make_noise(cfg, B, seed=12)
    before = {k: core.get("params", k).copy() for k in core.leaves}
    dry = core.eval_losses(db, AH.noise_to_device(cfg, noise))
    for k, v in before.items():
        assert _bits_equal(core.get("params", k), v), k
    core.update(db, noise=AH.noise_to_device(cfg, noise))
    info = core.read_info()
    for k, v in info.items():
        assert dry[k] == v, (k, dry[k], v)


# ---- the reference's own code --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MS.UPDATE_GOLDEN)
def test_hip_update_matches_the_reference_golden(gpu, name):
    """tests/test_golden_update_gpu.py::test_hip_update_matches_the_reference_golden on shapes_update_<name>.npz (injected noise)"""
    g = MS.load_golden(name)
    cfg = g["cfg"]
    agent = MS.reference_agent(cfg, g["B"])
    assert agent.core.critic_dims == cfg.critic_dims and agent.core.policy_dims == cfg.policy_dims
    AH.load_leaves(agent.core, cfg, *O.init_params(cfg, g["meta"]["param_seed"]))
    GR.replay(agent, g, label=f"shapes_update_{name}")
    assert agent.core.debug("ctr_nonzero", 1)[0] == 0


def test_reference_init_then_one_update_matches_the_reference(gpu):
    """tests/test_init_reference_gpu.py::test_reference_init_then_one_update_matches_the_reference on shapes_init_sac_state.npz:
    from the seed only, param_init="reference" """
    npz, cfg, recs, _ = MS.init_golden()
    g = G.unpack(npz)
    g["cfg"] = cfg
    agent = MS.reference_agent(cfg, g["B"], param_init="reference")
    core = agent.core
    assert core.critic_dims == (128, 64) and core.policy_dims == (64, 64, 128)
    bad = [m for n in sorted(recs) for sec in ("params", "target_params") for m in [IG.mismatch(n, recs[n], core.get(sec, n))] if m]
    assert not bad, bad
    for n in recs:
        for tx in ("critic", "actor", "temperature"):
            assert not core.get(f"opt/{tx}/mu", n).any() and not core.get(f"opt/{tx}/nu", n).any()
    assert [int(v) for v in agent.state.rng] == g["meta"]["rng0"] == [int(v) for v in npz["init_rng"]]
    assert [s["kind"] for s in g["steps"]] == ["high_utd"] and set(recs) == set(O.trainable_param_shapes(cfg))
    GR.replay(agent, g, seed_only=True, label="shapes_init_sac_state")
