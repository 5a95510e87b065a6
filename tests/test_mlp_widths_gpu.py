"""GPU: critic and policy MLPs of a width other than 256 (serl_agent_cfg.hidden, hidden_dims=[h, h]; a multiple of 64 in
[64, 1024]) -- the width-generic LayerNorm rows of serl_amd/csrc/heads.hip under the whole update chain.

* oracle parity of update_critics, update_high_utd (UTD 1 and one UTD > 1) and sample_actions at the widths of tests/mlp_widths.py
  (1, 3, 5, 8 and 16 columns per lane), every gradient leaf, the info scalars and the state after the step, at the tolerances of
  tests/test_agent_gpu.py (TOL = 1e-4, _compare_state);
* the fused chain against the one-launch-per-operation chain (SERL_CHAIN_FUSE 1 / 0) bit for bit on injected noise at 192 and 1024,
  with the launch count tests/test_chain_fusion_gpu.py pins for 256;
* the reference's own update code and initial parameters at widths 128 and 320 (tests/golden/widths_*.npz) with the comparisons and
  bounds of tests/test_golden_update_gpu.py and tests/test_init_reference_gpu.py;
* the data-parallel split, the checkpoint round trip and the refusals of the C ABI."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import drq_oracle as O
from oracle import golden_update as G
import agent_helpers as AH
import golden_replay as GR
import init_golden_helpers as IG
import mlp_widths as MW
from test_agent_gpu import TOL, _compare_state
from test_chain_fusion_gpu import _assert_state_bits, _bits_equal, _launches

pytestmark = pytest.mark.gpu


class _Figures:
    """every figure of a case is printed before the first assertion fails, so one run shows all of them"""

    def __init__(self, what):
        self.what, self.bad = what, []

    def add(self, name, err, tol=TOL):
        print(f"{self.what}: {name} = {err:.2e}")
        if not err < tol:
            self.bad.append((name, err))

    def check(self):
        assert not self.bad, (self.what, self.bad)


def _grads(fig, cfg, core, grads, tap):
    sl, _ = AH.leaf_slices(cfg)
    pc = sl.get("enc/proprio/ln/bias", sl["critic/head/bias"])[1]
    lo0 = 0 if tap == "g_critic" else sl.get("enc/proprio/dense/kernel", sl["actor/w1"])[0]
    g = core.debug(tap, {"g_critic": pc, "g_actor": sl["actor/logstd/bias"][1] - lo0}[tap])
    for k, gv in grads.items():
        lo, hi = sl[k]
        fig.add(f"{tap} {k}", AH.rel_err(g[lo - lo0:hi - lo0], gv.numpy().reshape(-1)))


def _info(fig, got, info, names):
    for k in names:
        fig.add(f"info {k}", abs(got[k] - info[k]) / max(1.0, abs(info[k])))


# ---- oracle parity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MW.CASES, ids=MW.IDS)
def test_update_critics_matches_the_oracle_at_width(gpu, case):
    cfg, B, _ = MW.case_config(case)
    st, core = AH.make_pair(cfg, B)
    assert core.cfg.hidden == cfg.hidden == case[1] and core.leaves["actor/w2"] == cfg.hidden * cfg.hidden
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


_UTD = [(c, 1) for c in MW.CASES] + [(c, c[5]) for c in MW.CASES if c[5] > 1]


@pytest.mark.parametrize("case,utd", _UTD, ids=[f"{c[0]}-utd{u}" for c, u in _UTD])
def test_update_high_utd_matches_the_oracle_at_width(gpu, case, utd):
    cfg, B, _ = MW.case_config(case)
    assert B % utd == 0
    st, core = AH.make_pair(cfg, B)
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


@pytest.mark.parametrize("case", MW.CASES, ids=MW.IDS)
def test_sample_actions_match_the_oracle_at_width(gpu, case):
    cfg, B, _ = MW.case_config(case)
    st, core = AH.make_pair(cfg, B)
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


# ---- fused against un-fused chain ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,kind,B,ensemble", [(192, "frozen", 65, 10), (1024, "frozen", 7, 3), (1024, "state", 65, 16)],
                         ids=["w192_frozen_B65", "w1024_frozen_B7", "w1024_state_B65_E16"])
def test_fused_chain_is_bit_identical_to_the_unfused_chain_at_width(gpu, h, kind, B, ensemble):
    cfg = MW.config(h, kind, ensemble)
    fused, plain = AH.make_pair(cfg, B, fuse=True)[1], AH.make_pair(cfg, B, fuse=False)[1]
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
            assert _bits_equal(fused.debug(tap, n), plain.debug(tap, n)), (h, kind, it, tap)
        fi, pi = fused.read_info(), plain.read_info()
        assert fi == pi, (h, kind, it, fi, pi)
        _assert_state_bits(cfg, fused, plain, (h, kind, it))
    print(f"width {h} {kind}: chain launches per update_critics + update_high_utd: fused {n_pair['fused']}, one-per-operation {n_pair['plain']}")
    if kind == "frozen":    # the pin of test_chain_fusion_gpu.py for 256: a critic + actor pair = 22 + 26 = 48 in the fused chain
        assert n_pair["plain"] >= 29 + 29 + 31, n_pair
        assert n_pair["fused"] <= 22 + 22 + 26, n_pair
    # ... and exactly what the same agent launches at 256 (state-only agents have no encoder launches: compared, not pinned)
    cfg256 = MW.config(256, kind, ensemble)
    for name, fuse in (("fused", True), ("plain", False)):
        core = AH.make_pair(cfg256, B, fuse=fuse)[1]
        db, dn = AH.batch_to_device(cfg256, AH.synth_batch(cfg256, B, seed=301)), AH.noise_to_device(cfg256, O.make_noise(cfg256, B, seed=401, utd_ratio=1))
        torch.cuda.synchronize()
        l0 = _launches()
        core.update_critics(db, dn)
        core.update_high_utd(db, 1, dn)
        torch.cuda.synchronize()
        assert _launches() - l0 == n_pair[name], (name, h, _launches() - l0, n_pair[name])
    assert fused.debug("ctr_nonzero", 1)[0] == 0


# ---- the reference's own code at other widths ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MW.UPDATE_GOLDEN)
def test_hip_update_matches_the_reference_golden_at_width(gpu, name):
    """tests/test_golden_update_gpu.py::test_hip_update_matches_the_reference_golden on widths_update_<name>.npz (injected noise)"""
    g = GR.load_variant("widths_update", name)[0]
    cfg = g["cfg"]
    agent = GR.reference_agent(cfg, g["B"])
    assert agent.core.cfg.hidden == cfg.hidden
    AH.load_leaves(agent.core, cfg, *O.init_params(cfg, g["meta"]["param_seed"]))
    GR.replay(agent, g, label=f"widths_update_{name}")
    assert agent.core.debug("ctr_nonzero", 1)[0] == 0


def test_reference_init_then_one_update_matches_the_reference_at_width_128(gpu):
    """tests/test_init_reference_gpu.py::test_reference_init_then_one_update_matches_the_reference on widths_init_sac_state_w128.npz:
    from the seed only, param_init="reference" """
    npz, cfg, recs, _ = MW.init_golden()
    g = G.unpack(npz)
    agent = GR.reference_agent(cfg, g["B"], param_init="reference")
    core = agent.core
    assert core.cfg.hidden == 128
    bad = [m for n in sorted(recs) for sec in ("params", "target_params") for m in [IG.mismatch(n, recs[n], core.get(sec, n))] if m]
    assert not bad, bad
    for n in recs:
        for tx in ("critic", "actor", "temperature"):
            assert not core.get(f"opt/{tx}/mu", n).any() and not core.get(f"opt/{tx}/nu", n).any()
    assert [int(v) for v in agent.state.rng] == g["meta"]["rng0"] == [int(v) for v in npz["init_rng"]]
    assert [s["kind"] for s in g["steps"]] == ["high_utd"] and set(recs) == set(O.trainable_param_shapes(cfg))
    GR.replay(agent, g, seed_only=True, label="widths_init_sac_state_w128")     # (cfg.lr = the 3e-4 of the init goldens' bound)


# ---- data-parallel split, checkpoints, the C ABI's refusals --------------------------------------------------------------------
def test_dp_split_equals_full_batch_at_width_192(gpu):
    """tests/test_agent_gpu.py::test_dp_split_equals_full_batch at hidden = 192: the gradients of two half batches (normalised by the
    global count) sum to the full-batch gradient"""
    cfg = MW.config(192, "frozen", 10)
    B = 16
    _, core = AH.make_pair(cfg, B)
    b = AH.synth_batch(cfg, B, seed=5)
    noise = AH.noise_to_device(cfg, O.make_noise(cfg, B, seed=9))
    db = AH.batch_to_device(cfg, b)
    sl, _ = AH.leaf_slices(cfg)
    n = sl["enc/proprio/ln/bias"][1]
    assert core.grad_view(1).numel() >= n      # (the view a data-parallel learner all-reduces is sized from the agent's leaves)
    core.begin_update()
    core.encode(db)
    core.critic_grads(0, B, B, noise)
    full = core.debug("g_critic", n).astype(np.float64)
    sc_full = core.debug("scalars", 3).astype(np.float64)
    parts, scs = [], []
    for r in range(2):
        core.critic_grads(r * 8, 8, B, noise)
        parts.append(core.debug("g_critic", n).astype(np.float64))
        scs.append(core.debug("scalars", 3).astype(np.float64))
    assert AH.rel_err(parts[0] + parts[1], full) < 1e-5
    assert AH.rel_err(scs[0] + scs[1], sc_full) < 1e-5


def _flat_batch(S, A, B, seed):
    r = np.random.default_rng(seed)
    return {"observations": r.standard_normal((B, S)).astype(np.float32), "next_observations": r.standard_normal((B, S)).astype(np.float32),
            "actions": r.uniform(-1, 1, (B, A)).astype(np.float32), "rewards": (r.random(B) < 0.3).astype(np.float32),
            "masks": (r.random(B) < 0.9).astype(np.float32)}


def _all_bits(agent):
    return {(sec, leaf): agent.core.get(sec, leaf).copy() for leaf in agent.core.leaves
            for sec in ("params", "target_params", "opt/critic/mu", "opt/critic/nu", "opt/actor/mu", "opt/actor/nu",
                        "opt/temperature/mu", "opt/temperature/nu")}


def test_checkpoint_roundtrip_at_width_128(gpu, tmp_path):
    """save_checkpoint(agent.state) at hidden = 128 -> restore into a fresh agent -> every leaf back and an identical next update;
    a checkpoint of a 256-wide agent is refused naming the leaf and both sizes, and leaves the agent untouched"""
    from serl_amd.utils.checkpoint import read_checkpoint_tree, restore_checkpoint, save_checkpoint
    S, A, B = 10, 4, 8
    agent = MW.sac_agent(128, seed=7, B=B, S=S, A=A)
    for i in range(2):
        agent.update_high_utd(_flat_batch(S, A, B, 10 + i), utd_ratio=2)
    save_checkpoint(str(tmp_path / "w128"), agent, step=agent.state.step)
    tree = read_checkpoint_tree(str(tmp_path / "w128"))
    assert tree["params"]["modules_actor"]["network"]["Dense_1"]["kernel"].shape == (128, 128)
    assert tree["params"]["modules_critic"]["network"]["Dense_0"]["kernel"].shape == (10, S + A, 128)
    fresh = MW.sac_agent(128, seed=1, B=B, S=S, A=A)
    restore_checkpoint(str(tmp_path / "w128"), fresh, restore_rng=True)
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
    # a 256-wide state into the 128-wide agent
    wide = MW.sac_agent(256, seed=7, B=B, S=S, A=A)
    wide.update_high_utd(_flat_batch(S, A, B, 10), utd_ratio=2)
    save_checkpoint(str(tmp_path / "w256"), wide, step=wide.state.step)
    before, step_before = _all_bits(fresh), fresh.state.step
    with pytest.raises(ValueError, match=r"leaf '[a-z0-9/]+' has \d+ elements in this agent, the state holds \d+") as e:
        restore_checkpoint(str(tmp_path / "w256"), fresh)
    leaf = str(e.value).split("'")[1]
    assert f"has {fresh.core.leaves[leaf]} elements" in str(e.value) and f"holds {wide.core.leaves[leaf]} " in str(e.value)
    assert fresh.core.leaves[leaf] != wide.core.leaves[leaf]
    assert fresh.state.step == step_before
    for key, v in _all_bits(fresh).items():
        assert _bits_equal(v, before[key]), ("touched by the refused restore", key)


def _create(hidden=256, bottleneck=256):
    """serl_agent_create with a state-only configuration -> (status, serl_last_error())"""
    from serl_amd import _lib
    from serl_amd._lib_agent import SerlAgentCfg
    L = _lib.lib()
    cfg = SerlAgentCfg(0, 0, 0, 0, 10, 4, 8, 10, hidden, bottleneck, 8, 64, 0, -1, 0.99, 0.005, 3e-4, 0.1, 1e-5, 5.0, -2.0, 0)
    h = C.c_void_p()
    rc = int(L.serl_agent_create(C.byref(cfg), C.byref(h)))
    msg = (L.serl_last_error() or b"").decode()
    if rc == 0:
        assert int(L.serl_agent_destroy(h)) == 0
    return rc, msg


def test_c_abi_refusals(gpu):
    SERL_ERR_INVALID = -1      # include/serl_mi355.h
    for h in (0, 100, 1088, -64, 32):
        rc, msg = _create(hidden=h)
        assert rc == SERL_ERR_INVALID and f"hidden must be a multiple of 64 in [64, 1024] (got {h})" in msg, (h, rc, msg)
    rc, msg = _create(bottleneck=128)
    assert rc == SERL_ERR_INVALID and "bottleneck must be 256 (got 128)" in msg and "hidden" not in msg, (rc, msg)
    for h in (64, 256, 1024):
        rc, msg = _create(hidden=h)
        assert rc == 0, (h, rc, msg)
