"""GPU: critic and policy MLP widths off the 64 grid (serl_agent_opts.ragged_widths, mlp_ragged=True) under the whole update chain,
on the case table of tests/mlp_ragged.py.  The ragged rows are the RAGGED instantiations of ln_row / ln_bwd_row (csrc/heads.hip):
a layer of true width d is stored 64 ceil(d / 64) wide in zero padding, its LayerNorm divides by d and its backward leaves dx = 0
in the pads.  The plain rows are the ones every agent launches.

* oracle parity of update_critics and update_high_utd (UTD 1 and the table's) in both schedules of the chain: info scalars, q,
  target_q, next log-prob, every gradient leaf, the state after the step, with the helpers and at the tolerances of
  tests/test_mlp_shapes_gpu.py and tests/test_mlp_plain_gpu.py (TOL = 1e-4, _compare_state); the gradient taps are read through the
  storage layout (mlp_ragged.grads), and their padding is asserted to be zero on the way;
* widths on the grid through the option against the call without, bit for bit; launch counts against the agent of the padded widths;
* the pad invariant (debug tap "pad_max_abs") after creation, after a set of every leaf in every section, after AdamW + clipped
  updates; get(set(x)) == x for every leaf and section;
* snapshots, a checkpoint round trip and the refusals across widths; the read-only calls; two shards against the full batch.

Without the option every test here fails when its agent is made (AgentCore has no `ragged`, create_states no `mlp_ragged`)."""
import numpy as np
import pytest
import torch

from oracle import drq_oracle as O
import agent_helpers as AH
import eval_oracle as EO
import mlp_ragged as MR
import mlp_shapes as MS
import policy_fixed as PF
from test_agent_gpu import TOL, _compare_state
from test_chain_fusion_gpu import _assert_state_bits, _bits_equal, _launches
from test_mlp_widths_gpu import _Figures, _flat_batch, _info

pytestmark = pytest.mark.gpu
FUSE = pytest.mark.parametrize("fuse", [True, False], ids=["fused", "unfused"])


@pytest.fixture(autouse=True)
def _general_oracle():
    with MR.installed():
        yield


def _core_of(run, fuse, ragged=True):
    """a fresh agent holding the parameters the case's oracle run started from"""
    cfg = run["cfg"]
    trunk, theta = PF.init_params(cfg, run["seed"])
    return AH.load_leaves(MR.make_core(cfg, run["B"], fuse=fuse, ragged=ragged), cfg, trunk, theta)


def _true_shapes(core, cfg):
    assert core.critic_dims == cfg.critic_dims and core.policy_dims == cfg.policy_dims
    fan = ([cfg.enc_dim] + list(cfg.policy_dims))
    assert core.leaves[f"actor/w{len(cfg.policy_dims)}"] == fan[-2] * fan[-1]
    assert core.leaves["actor/mean/kernel"] == cfg.policy_dims[-1] * cfg.A
    assert core.leaves["critic/head/kernel"] == (cfg.ensemble if cfg.state_only else 1) * cfg.critic_dims[-1]
    assert core.leaves["critic/b1"] == cfg.ensemble * cfg.critic_dims[0]


# ---- 1 - 6: oracle parity, both schedules of the chain ---------------------------------------------------------------------------
@FUSE
@pytest.mark.parametrize("name", MR.IDS)
def test_update_critics_matches_the_oracle(gpu, name, fuse):
    run = MR.oracle_run(name, "critics")
    cfg, B, st, aux = run["cfg"], run["B"], run["state"], run["aux"]
    core = _core_of(run, fuse)
    _true_shapes(core, cfg)
    assert core.pad_max_abs == 0.0
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
    assert core.debug("ctr_nonzero", 1)[0] == 0 and core.pad_max_abs == 0.0


_UTD = [(n, 1) for n in MR.IDS] + [(n, MR.CASES[n]["utd"]) for n in MR.IDS if MR.CASES[n]["utd"] > 1]


@FUSE
@pytest.mark.parametrize("name,utd", _UTD, ids=[f"{n}-utd{u}" for n, u in _UTD])
def test_update_high_utd_matches_the_oracle(gpu, name, utd, fuse):
    run = MR.oracle_run(name, ("high_utd", utd))
    cfg, B, st = run["cfg"], run["B"], run["state"]
    assert B % utd == 0
    core = _core_of(run, fuse)
    core.update_high_utd(AH.batch_to_device(cfg, run["batch"]), utd, AH.noise_to_device(cfg, run["noise"]))
    fig = _Figures(f"update_high_utd({utd}) {name} {'fused' if fuse else 'unfused'}")
    _info(fig, core.read_info(), run["info"], ("critic_loss", "predicted_qs", "target_qs", "actor_loss", "temperature", "entropy", "temperature_loss"))
    MR.grads(fig, cfg, core, run["aux"]["g_actor"], "g_actor")
    if cfg.fixed_std is not None:      # TD3 as the reference writes it: the std of the actor phase's evaluation is clip(fixed_std), in float32
        std = core.debug("std", B * cfg.A).reshape(B, cfg.A)
        want = np.clip(np.asarray(cfg.fixed_std, np.float32), np.float32(cfg.std_min), np.float32(cfg.std_max))
        assert np.array_equal(std, np.broadcast_to(want, std.shape)) and "actor/logstd/kernel" not in core.leaves
    fig.check()
    _compare_state(cfg, st, core, steps=utd + 1)
    assert core.step == st.step == utd + 1
    assert core.debug("ctr_nonzero", 1)[0] == 0 and core.pad_max_abs == 0.0


@pytest.mark.parametrize("name", ["r1_state_400_300", "r4_state_one_layer_critic_200", "r6_frozen_100_200__300"])
def test_fused_chain_is_bit_identical_to_the_unfused_chain(gpu, name):
    cfg, B, _, seed = MR.case_config(name)
    fused, unfused = MR.make_pair(cfg, B, seed=seed, fuse=True)[1], MR.make_pair(cfg, B, seed=seed, fuse=False)[1]
    rng = MR.tap_ranges(fused)
    for it in range(2):
        b = AH.synth_batch(cfg, B, seed=300 + it)
        noise = O.make_noise(cfg, B, seed=400 + it, utd_ratio=1)
        for core in (fused, unfused):
            db, dn = AH.batch_to_device(cfg, b), AH.noise_to_device(cfg, noise)
            core.update_critics(db, dn)
            core.update_high_utd(db, 1, dn)
        for tap, n in (("g_critic", rng["g_critic"][1]), ("g_actor", rng["g_actor"][1] - rng["g_actor"][0]), ("scalars", 8),
                       ("q", cfg.ensemble * B), ("target_q", B), ("logp", B), ("dx", B * (cfg.enc_dim + cfg.A))):
            assert _bits_equal(fused.debug(tap, n), unfused.debug(tap, n)), (name, it, tap)
        assert fused.read_info() == unfused.read_info()
        _assert_state_bits(cfg, fused, unfused, (name, it))
    assert fused.debug("ctr_nonzero", 1)[0] == 0 and fused.pad_max_abs == 0.0 and unfused.pad_max_abs == 0.0


# ---- 7: widths on the grid through the option ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,cd,pd", [("state", (128, 256, 64), (192,)), ("frozen1", (320,), (64, 256))], ids=["state", "frozen1"])
def test_widths_on_the_grid_through_the_option_are_the_agent_without_it(gpu, kind, cd, pd):
    B = 6
    cfg = PF.FixedConfig(**MS.config(kind, cd, pd, ensemble=3).__dict__)
    with_opt, without = MR.make_pair(cfg, B, ragged=True)[1], MR.make_pair(cfg, B, ragged=False)[1]
    assert with_opt.spec.to_c().ragged_widths == 1 and without.spec.to_c().ragged_widths == 0
    assert list(with_opt.leaves.items()) == list(without.leaves.items())
    assert all(with_opt.leaf_layout(k) == without.leaf_layout(k) for k in with_opt.leaves)
    n = {}
    for it in range(2):
        b = AH.synth_batch(cfg, B, seed=300 + it)
        noise = O.make_noise(cfg, B, seed=400 + it, utd_ratio=2)
        for label, core in (("with", with_opt), ("without", without)):
            db, dn = AH.batch_to_device(cfg, b), AH.noise_to_device(cfg, noise)
            torch.cuda.synchronize()
            l0 = _launches()
            core.update_high_utd(db, 2, dn)
            torch.cuda.synchronize()
            n[label] = _launches() - l0
        assert with_opt.read_info() == without.read_info()
        _assert_state_bits(cfg, with_opt, without, (kind, it))
    assert n["with"] == n["without"], n
    assert with_opt.pad_max_abs == 0.0


# ---- 8: the launches are those of the padded widths ---------------------------------------------------------------------------------
@FUSE
def test_ragged_agent_launches_what_the_agent_of_the_padded_widths_launches(gpu, fuse):
    cfg, B, _, _ = MR.case_config("r1_state_400_300")
    grid = PF.FixedConfig(**{**cfg.__dict__, "critic_dims": (448, 320), "policy_dims": (448, 320), "hidden": 448})
    n = {}
    b, noise = AH.synth_batch(cfg, B, seed=310), O.make_noise(cfg, B, seed=410, utd_ratio=1)
    for label, c in (("ragged", cfg), ("grid", grid)):
        core = MR.make_pair(c, B, fuse=fuse)[1]
        db, dn = AH.batch_to_device(c, b), AH.noise_to_device(c, noise)
        torch.cuda.synchronize()
        l0 = _launches()
        core.update_critics(db, dn)
        core.update_high_utd(db, 1, dn)
        torch.cuda.synchronize()
        n[label] = _launches() - l0
    print(f"chain launches per update_critics + update_high_utd(1), {'fused' if fuse else 'unfused'}: {n}")
    assert n["ragged"] == n["grid"], n


# ---- 9, 10: the pad invariant; get(set(x)) == x ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["r1_state_400_300", "r4_state_one_layer_critic_200", "r5_state_plain_relu_critic_beside_ln_swish_policy",
                                  "r6_small_100_200__300"])
def test_padding_is_zero_after_creation_set_and_adamw_updates(gpu, name):
    cfg, B, _, seed = MR.case_config(name)
    cfg.opt = {k: {"learning_rate": 3e-3, "weight_decay": 1e-2, "clip_grad_norm": 0.5} for k in ("actor", "critic", "temperature")}
    core = MR.make_core(cfg, B)
    assert any(lay[4] != lay[2] or lay[3] != lay[1] for lay in map(core.leaf_layout, core.leaves)), "no leaf of this case is padded"
    assert core.pad_max_abs == 0.0                                                   # after creation
    rng = np.random.default_rng(5)
    written = {}
    for leaf, n in core.leaves.items():
        if leaf.startswith("trunk/"):
            continue
        for sec in MR.SECTIONS:
            x = (rng.standard_normal(n) + 3.0).astype(np.float32)                    # (no element is zero)
            try:
                core.set(sec, leaf, x)
                written[sec, leaf] = x
            except Exception as e:      # a moment outside its optimizer's support takes zeros alone
                assert "outside the optimizer's support" in str(e), (sec, leaf, e)
                core.set(sec, leaf, np.zeros(n, np.float32))
                written[sec, leaf] = np.zeros(n, np.float32)
    assert core.pad_max_abs == 0.0                                                   # after a set of every leaf in every section
    for (sec, leaf), x in written.items():
        assert _bits_equal(core.get(sec, leaf), x), (sec, leaf)                      # get(set(x)) == x, at true shapes
    trunk, theta = PF.init_params(cfg, seed)
    AH.load_leaves(core, cfg, trunk, theta)
    for sec in MR.SECTIONS[2:]:
        for leaf, n in core.leaves.items():
            if not leaf.startswith("trunk/"):
                core.set(sec, leaf, np.zeros(n, np.float32))
    for it in range(3):
        core.update_high_utd(AH.batch_to_device(cfg, AH.synth_batch(cfg, B, seed=20 + it)), 2,
                             AH.noise_to_device(cfg, O.make_noise(cfg, B, seed=30 + it, utd_ratio=2)))
    info = core.read_info()
    assert all(np.isfinite(v) for v in info.values()), info
    assert core.pad_max_abs == 0.0                                                   # after three AdamW updates with a clip
    moved = max(float(np.abs(core.get("params", k) - np.asarray(v, np.float32).reshape(-1)).max()) for k, v in theta.items()
                if k.startswith("critic/w"))
    assert moved > 0.0


def test_leaf_layout_states_the_padded_box(gpu):
    cfg, B, _, _ = MR.case_config("r1_state_400_300")
    core = MR.make_core(cfg, B)
    E = cfg.ensemble
    assert core.leaf_layout("critic/w1") == (E, cfg.S + cfg.A, 400, cfg.S + cfg.A, 448)
    assert core.leaf_layout("critic/w2") == (E, 400, 300, 448, 320)
    assert core.leaf_layout("critic/ln2/scale") == (E, 1, 300, 1, 320)
    assert core.leaf_layout("critic/head/kernel") == (E, 1, 300, 1, 320)
    assert core.leaf_layout("actor/mean/kernel") == (1, 300, cfg.A, 320, cfg.A)
    n, rows, cols, rows_p, ld = core.leaf_layout("temp/lagrange")
    assert n * rows * cols == 1 == n * rows_p * ld
    total = sum(lay[0] * lay[3] * lay[4] for lay in map(core.leaf_layout, core.leaves))
    assert core.grad_view(7).numel() == total - 1 + 32       # [critic grads | 32 scalars | actor grads]: the storage, without the temperature


# ---- 11: snapshots, checkpoints, refusals across widths ---------------------------------------------------------------------------
def test_snapshot_leaves_equal_get_and_checkpoint_roundtrip(gpu, tmp_path):
    from serl_amd.utils.checkpoint import load_state_dict, read_checkpoint_tree, restore_checkpoint, save_checkpoint
    S, A, B = 10, 4, 8
    cd, pd = (100, 50), (65,)
    agent = MR.sac_agent(cd, pd, seed=7, B=B, S=S, A=A)
    assert agent.core.critic_dims == cd and agent.core.policy_dims == pd and agent.core.spec.ragged
    for i in range(2):
        agent.update_high_utd(_flat_batch(S, A, B, 10 + i), utd_ratio=2)
    tree = agent.state.params
    assert tree["modules_critic"]["network"]["Dense_1"]["kernel"].shape == (10, 100, 50)
    assert tree["modules_actor"]["network"]["LayerNorm_0"]["scale"].shape == (65,)
    with agent.snapshot(("params", "target_params", "opt_states")) as snap:
        assert snap.finite
        for sec in ("params", "target_params", "opt/critic/mu", "opt/actor/nu"):
            for leaf in agent.core.leaves:
                got = snap._get(sec, leaf)
                assert got.size == agent.core.leaves[leaf] and _bits_equal(np.ascontiguousarray(got).reshape(-1), agent.core.get(sec, leaf)), (sec, leaf)
        sd = {"params": snap.params, "target_params": snap.target_params, "opt_states": snap.opt_states, "step": snap.step}
        assert sd["params"]["modules_critic"]["network"]["Dense_1"]["kernel"].shape == (10, 100, 50)
        fresh = MR.sac_agent(cd, pd, seed=1, B=B, S=S, A=A)
        load_state_dict(fresh, sd)
    fresh._rng_key = agent._rng_key.copy()
    want = MR.all_bits(agent.core)
    for key, v in MR.all_bits(fresh.core).items():
        assert _bits_equal(v, want[key]), key
    save_checkpoint(str(tmp_path / "ragged"), agent, step=agent.state.step)
    assert read_checkpoint_tree(str(tmp_path / "ragged"))["params"]["modules_actor"]["network"]["Dense_0"]["kernel"].shape == (S, 65)
    again = MR.sac_agent(cd, pd, seed=2, B=B, S=S, A=A)
    restore_checkpoint(str(tmp_path / "ragged"), again, restore_rng=True)
    nxt = _flat_batch(S, A, B, 20)
    for a in (agent, fresh, again):
        a.update_high_utd(nxt, utd_ratio=1)
    want = MR.all_bits(agent.core)
    for other in (fresh, again):
        for key, v in MR.all_bits(other.core).items():
            assert _bits_equal(v, want[key]), ("after the next update", key)
    assert agent.core.pad_max_abs == 0.0 and fresh.core.pad_max_abs == 0.0 and again.core.pad_max_abs == 0.0
    # other widths, both ways: the storage of (100, 50) and of (128, 64) is the same, the leaves are not
    wide = MS.sac_agent((128, 64), (128,), seed=3, B=B, S=S, A=A)
    for src, dst in ((agent, wide), (wide, agent)):
        before, step_before = MR.all_bits(dst.core), dst.state.step
        state = {"params": src.state.params, "target_params": src.state.target_params, "opt_states": src.state.opt_states, "step": 5}
        with pytest.raises(ValueError, match=r"leaf '[a-z0-9/]+' has \d+ elements in this agent, the state holds \d+"):
            load_state_dict(dst, state)
        assert dst.state.step == step_before
        for key, v in MR.all_bits(dst.core).items():
            assert _bits_equal(v, before[key]), ("touched by the refused restore", key)


# ---- 12: the read-only calls ------------------------------------------------------------------------------------------------------
def test_read_only_calls_against_the_restatement(gpu):
    import trained_regime as TR
    from test_evaluate_gpu import _check, _core_eval, _dev
    cfg, B, _, seed = MR.case_config("r2_state_65_127")
    trunk, theta = PF.init_params(cfg, seed)
    target = TR.perturb_target(theta, cfg)
    core = AH.load_leaves(MR.make_core(cfg, B), cfg, trunk, theta, target)
    rng = np.random.default_rng(5)
    state = rng.standard_normal((B, cfg.S)).astype(np.float32)
    act = EO.scaled_actions(rng.uniform(-1, 1, (B, cfg.A)))
    ref64, err32 = EO.log_prob_yardstick(cfg, trunk, theta, target, {}, state, act)
    before = MR.all_bits(core)
    got = _core_eval(core, None, _dev(state), _dev(act))
    _check("r2_state_65_127", got, ref64, err32)
    assert AH.rel_err(ref64["q"], ref64["q_target"]) > 1e-3
    # the mode is the argmax action, and the std is the std of an update's own policy forward on the same rows, bit for bit
    assert np.array_equal(got["mode"], core.sample_actions(None, _dev(state), None).cpu().numpy())
    b = AH.synth_batch(cfg, B, seed=2)
    db, dn = AH.batch_to_device(cfg, b), AH.noise_to_device(cfg, O.make_noise(cfg, B, seed=3))
    mine = core.eval_policy(None, db.state[0], None)["std"].cpu().numpy()
    dry = core.eval_losses(db, dn)
    for key, v in MR.all_bits(core).items():
        assert _bits_equal(v, before[key]), ("a read-only call wrote", key)
    core.update(db, ("actor", "critic", "temperature"), dn)
    assert np.array_equal(mine.reshape(-1), core.debug("std", B * cfg.A))
    info = core.read_info()
    for k in dry:
        assert np.float32(dry[k]).tobytes() == np.float32(info[k]).tobytes(), (k, dry[k], info[k])


def test_evaluate_losses_against_the_oracle(gpu):
    cfg, B, _, seed = MR.case_config("r2_state_65_127")
    st, core = MR.make_pair(cfg, B, seed=seed)
    b, noise = AH.synth_batch(cfg, B, seed=6), O.make_noise(cfg, B, seed=9)
    tb, tn = AH.batch_to_torch(b, torch.float64), O.noise_to_torch(noise, torch.float64)
    tn["redq_idx"] = np.asarray(noise["redq_idx"]).reshape(-1, cfg.subsample)[0]
    fo, fn = O.features(st, tb["obs"]), O.features(st, tb["next"])
    ci, _ = O.critic_update(st, fo, fn, tb["state"], tb["next_state"], tb["action"], tb["reward"], tb["mask"], tn, apply=False)
    ai, _ = O.actor_temp_update(st, fo, fn, tb["state"], tb["next_state"], tn, apply=False)
    got = core.eval_losses(AH.batch_to_device(cfg, b), AH.noise_to_device(cfg, noise))
    for k, v in {**ci, **ai}.items():
        print("evaluate_losses r2", k, got[k], v)
        assert abs(got[k] - v) <= TOL * max(1.0, abs(v)), (k, got[k], v)


# ---- 13: two shards against the full batch, through the phase API ------------------------------------------------------------------
def test_two_shards_equal_the_full_batch(gpu):
    cfg, B, _, seed = MR.case_config("r1_state_400_300")
    _, core = MR.make_pair(cfg, B, seed=seed)
    noise = AH.noise_to_device(cfg, O.make_noise(cfg, B, seed=9))
    db = AH.batch_to_device(cfg, AH.synth_batch(cfg, B, seed=5))
    n = MR.tap_ranges(core)["g_critic"][1]
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
    st = MR.storage(core)
    for k, entry in st.items():
        if entry[0] < n:
            assert not MR.pads(parts[0] + parts[1], 0, entry).any(), k       # what an all-reduce sums stays zero in the padding
    assert core.pad_max_abs == 0.0


# ---- the reference's own code (tests/golden/ragged_*.npz) ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", MR.UPDATE_GOLDEN)
def test_hip_update_matches_the_reference_golden(gpu, name):
    """tests/test_mlp_shapes_gpu.py::test_hip_update_matches_the_reference_golden on ragged_update_<name>.npz (injected noise)"""
    import golden_replay as GR
    g = MR.load_golden(name)
    cfg = g["cfg"]
    agent = MR.reference_agent(cfg, g["B"])
    assert agent.core.critic_dims == cfg.critic_dims and agent.core.policy_dims == cfg.policy_dims and agent.core.spec.ragged
    AH.load_leaves(agent.core, cfg, *O.init_params(cfg, g["meta"]["param_seed"]))
    GR.replay(agent, g, label=f"ragged_update_{name}")
    assert agent.core.debug("ctr_nonzero", 1)[0] == 0 and agent.core.pad_max_abs == 0.0


def test_reference_init_then_one_update_matches_the_reference(gpu):
    """tests/test_mlp_shapes_gpu.py::test_reference_init_then_one_update_matches_the_reference on ragged_init_sac_state.npz: from the
    seed only, param_init="reference" """
    import golden_replay as GR
    import init_golden_helpers as IG
    from oracle import golden_update as G
    npz, cfg, recs, _ = MR.init_golden()
    g = G.unpack(npz)
    g["cfg"] = cfg
    agent = MR.reference_agent(cfg, g["B"], param_init="reference")
    core = agent.core
    assert core.critic_dims == (100, 50) and core.policy_dims == (65, 127, 3) and core.pad_max_abs == 0.0
    bad = [m for n in sorted(recs) for sec in ("params", "target_params") for m in [IG.mismatch(n, recs[n], core.get(sec, n))] if m]
    assert not bad, bad
    assert [int(v) for v in agent.state.rng] == g["meta"]["rng0"] == [int(v) for v in npz["init_rng"]]
    assert [s["kind"] for s in g["steps"]] == ["high_utd"] and set(recs) == set(O.trainable_param_shapes(cfg))
    GR.replay(agent, g, seed_only=True, label="ragged_init_sac_state")
    assert core.pad_max_abs == 0.0


def test_pad_tap_sees_every_kind_of_padding(gpu):
    """a value written into one pad float of the gradient buffers (debug_set writes storage) is what "pad_max_abs" reads: a pad
    column of a vector, a pad row of a kernel whose own width is on the grid (actor/w4 of [3, 200, 100, 64]: 100 rows in 128) and
    a pad row of the mean head's kernel -- one-block leaves with ld == cols, whose elements are one contiguous run"""
    cfg, B, _, _ = MR.case_config("r4_state_one_layer_critic_200")
    core = MR.make_core(cfg, B)
    st, rng = MR.storage(core), MR.tap_ranges(core)
    assert core.leaf_layout("actor/w4") == (1, 100, 64, 128, 64) and core.leaf_layout("actor/mean/kernel") == (1, 64, cfg.A, 64, cfg.A)
    assert core.leaf_layout("actor/w2") == (1, 3, 200, 64, 256)
    spots = [("g_critic", "critic/b1", 200), ("g_critic", "critic/head/kernel", 255), ("g_actor", "actor/w4", 100 * 64 + 5),
             ("g_actor", "actor/w4", 128 * 64 - 1), ("g_actor", "actor/w2", 3 * 256), ("g_actor", "actor/w2", 199 + 1)]
    for k, (tap, leaf, at) in enumerate(spots):
        lo, hi = rng[tap]
        flat = np.zeros(hi - lo, np.float32)
        flat[st[leaf][0] - lo + at] = 2.0 + k
        assert MR.pads(flat, lo, st[leaf]).max() == 2.0 + k and not MR.cut(flat, lo, st[leaf]).any(), (tap, leaf, at)
        core.debug_set(tap, flat)
        assert core.pad_max_abs == 2.0 + k, (tap, leaf, at)
        core.debug_set(tap, np.zeros(hi - lo, np.float32))
        assert core.pad_max_abs == 0.0
    # the mean head's pad rows, in an agent whose last policy width is off the grid
    cfg, B, _, _ = MR.case_config("r1_state_400_300")
    core = MR.make_core(cfg, B)
    st, (lo, hi) = MR.storage(core), MR.tap_ranges(core)["g_actor"]
    for leaf in ("actor/mean/kernel", "actor/logstd/kernel"):
        assert core.leaf_layout(leaf) == (1, 300, cfg.A, 320, cfg.A)
        flat = np.zeros(hi - lo, np.float32)
        flat[st[leaf][0] - lo + 300 * cfg.A] = -7.0
        core.debug_set("g_actor", flat)
        assert core.pad_max_abs == 7.0, leaf
        core.debug_set("g_actor", np.zeros(hi - lo, np.float32))
    assert core.pad_max_abs == 0.0
