"""GPU: the policy distributions beside the launcher's -- std_parameterization "softplus" and "uniform" and the unsquashed
Gaussian (serl_agent_create_policy's std_param / no_tanh; the MODE template parameter of the head kernels in serl_amd/csrc/heads.hip).

* the reference's own update code in every new mode (tests/golden/policy_*.npz, injected noise) with the comparisons and bounds of
  tests/golden_replay.py::replay, walked over the agent's own leaves (a uniform agent has actor/log_stds and no
  log-std Dense), at 72 rows (two head tiles, the second ragged) and A = 5; two of them in the regime where whole std columns clip;
* sample_actions, mode and injected noise, against the float64 head of oracle/drq_oracle.py;
* the fused chain against the one-launch-per-operation chain bit for bit at hidden = 192, 65 rows, and a uniform agent's launch count
  against the exp agent's;
* the checkpoint round trip of a uniform agent, and the refusal of an exp state;
* the C ABI: serl_agent_create and its struct build the agent they always did, serl_agent_create_policy range-checks its arguments."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from oracle import drq_oracle as O
import agent_helpers as AH
import golden_replay as GR
import mlp_widths as MW
import policy_modes as PM
from test_agent_gpu import TOL
from test_chain_fusion_gpu import _assert_state_bits, _bits_equal, _launches
from test_mlp_widths_gpu import _all_bits, _flat_batch

pytestmark = pytest.mark.gpu


# ---- the reference's own code in every new mode ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PM.GOLDEN))
def test_hip_update_matches_the_reference_golden_in_mode(gpu, name):
    g, meta, _ = GR.load_variant("policy", name)
    cfg, B = g["cfg"], g["B"]
    std, squash = meta["policy"]["std_parameterization"], meta["policy"]["tanh_squash_distribution"]
    assert (std, squash) == PM.GOLDEN[name][3] and B == PM.GOLDEN[name][1] and cfg == PM.GOLDEN[name][0]
    agent = GR.reference_agent(cfg, B, policy_kwargs=PM.policy_kwargs(std, squash))
    assert ("actor/log_stds" in agent.core.leaves) == (std == "uniform") == ("actor/logstd/kernel" not in agent.core.leaves)
    AH.load_leaves(agent.core, cfg, *PM.initial_leaves(name))
    GR.replay(agent, g, label=f"policy_{name}")
    assert agent.core.debug("ctr_nonzero", 1)[0] == 0


# ---- sample_actions ------------------------------------------------------------------------------------------------------------
def _core(cfg, B, std, squash, theta, trunk=None, fuse=None):
    """AgentCore of this distribution holding `theta` (oracle names) in params and target_params"""
    cfg = dataclasses.replace(cfg, std_parameterization=std, tanh_squash=squash)
    return AH.load_leaves(AH.make_core(cfg, B, fuse=fuse), cfg, trunk, theta)


@pytest.mark.parametrize("std,squash", [PM.DEFAULT_MODE] + PM.NEW_MODES, ids=["exp"] + PM.MODE_IDS)
def test_sample_actions_match_the_float64_head_in_mode(gpu, std, squash):
    cfg, B = O.Config(image_keys=(), S=10, A=5, discount=0.99), 72
    theta = PM.mode_theta(O.init_params(cfg, GR.PARAM_SEED)[1], cfg, std, "init")
    core = _core(cfg, B, std, squash, theta)
    rng = np.random.default_rng(6)
    state = rng.standard_normal((B, cfg.S)).astype(np.float32)
    eps = (2.0 * rng.standard_normal((B, cfg.A))).astype(np.float32)      # (wide enough that unsquashed samples leave [-1, 1])
    th = O.to_torch(theta, torch.float64)
    mean, sd = O.policy_head(th, dataclasses.replace(cfg, std_parameterization=std), torch.tensor(state, dtype=torch.float64))
    dstate = torch.tensor(state, device="cuda")
    mode = core.sample_actions(None, dstate, None).cpu().numpy()
    want_mode = (torch.tanh(mean) if squash else mean).numpy()
    e_mode = AH.rel_err(mode, want_mode)
    got = core.sample_actions(None, dstate, torch.tensor(eps, device="cuda")).cpu().numpy()
    want, _ = O.sample_and_log_prob(mean, sd, torch.tensor(eps, dtype=torch.float64), squash)
    e_sample = AH.rel_err(got, want.numpy())
    print(f"sample_actions {std} squash={squash}: mode {e_mode:.2e}, sample {e_sample:.2e}, max |a| {np.abs(got).max():.3f}")
    assert e_mode < TOL and e_sample < TOL
    if squash:
        assert np.abs(got).max() <= 1.0 and np.abs(mode).max() <= 1.0
    else:
        assert (np.abs(want.numpy()) > 1.0).any() and (np.abs(got) > 1.0).any()
    assert core.debug("ctr_nonzero", 1)[0] == 0


# ---- fused against un-fused chain ----------------------------------------------------------------------------------------------
def _spans(core):
    """-> {leaf: (lo, hi)} of the trainable arena, from the agent's own leaf table"""
    sl, off = {}, 0
    for k, n in core.leaves.items():
        if k.startswith("trunk/"):
            continue
        sl[k] = (off, off + n)
        off += n
    return sl


def _pair_launches(core, cfg, B, b, noise):
    db, dn = AH.batch_to_device(cfg, b), AH.noise_to_device(cfg, noise)
    torch.cuda.synchronize()
    l0 = _launches()
    core.update_critics(db, dn)
    core.update_high_utd(db, 1, dn)
    torch.cuda.synchronize()
    return _launches() - l0


_FUSE_CASES = [(s, t, "state") for s, t in PM.NEW_MODES] + [("uniform", True, "frozen")]


@pytest.mark.parametrize("std,squash,kind", _FUSE_CASES, ids=[f"{i}-state" for i in PM.MODE_IDS] + ["uniform-frozen"])
def test_fused_chain_is_bit_identical_to_the_unfused_chain_in_mode(gpu, std, squash, kind):
    cfg, B = MW.config(192, kind, 10), 65
    trunk, theta0 = O.init_params(cfg, GR.PARAM_SEED)
    theta = PM.mode_theta(theta0, cfg, std, "init")
    fused, plain = (_core(cfg, B, std, squash, theta, trunk, fuse=f) for f in (True, False))
    sl = _spans(fused)
    last_actor = "actor/log_stds" if std == "uniform" else "actor/logstd/bias"
    pc = sl.get("enc/proprio/ln/bias", sl["critic/head/bias"])[1]
    pa0, pa1 = sl.get("enc/proprio/dense/kernel", sl["actor/w1"])[0], sl[last_actor][1]
    n_pair = {}
    for it in range(2):
        b = AH.synth_batch(cfg, B, seed=300 + it)
        noise = O.make_noise(cfg, B, seed=400 + it, utd_ratio=1)
        for name, core in (("fused", fused), ("plain", plain)):
            n_pair[name] = _pair_launches(core, cfg, B, b, noise)
        for tap, n in (("g_critic", pc), ("g_actor", pa1 - pa0), ("scalars", 8), ("q", cfg.ensemble * B), ("target_q", B), ("logp", B),
                       ("dx", B * (cfg.enc_dim + cfg.A))):
            assert _bits_equal(fused.debug(tap, n), plain.debug(tap, n)), (std, squash, it, tap)
        g_ls = fused.debug("g_actor", pa1 - pa0)[sl[last_actor][0] - pa0:]
        assert g_ls.size == cfg.A and np.abs(g_ls).min() > 0, g_ls      # (the log-std gradient is there, in every column)
        fi, pi = fused.read_info(), plain.read_info()
        assert fi == pi, (std, squash, it, fi, pi)
        _assert_state_bits(cfg, fused, plain, (std, squash, it))
    # a uniform agent's head is one GEMM group less, never a launch more: against the exp agent at the same shape
    for name, fuse in (("fused", True), ("plain", False)):
        ref = _core(cfg, B, "exp", True, theta0, trunk, fuse=fuse)
        n_exp = _pair_launches(ref, cfg, B, AH.synth_batch(cfg, B, seed=301), O.make_noise(cfg, B, seed=401, utd_ratio=1))
        print(f"{std} squash={squash} {kind}: {name} chain launches per critic + actor pair {n_pair[name]}, exp agent {n_exp}")
        assert n_pair[name] <= n_exp, (name, n_pair[name], n_exp)
    assert fused.debug("ctr_nonzero", 1)[0] == 0 and plain.debug("ctr_nonzero", 1)[0] == 0


# ---- checkpoints ---------------------------------------------------------------------------------------------------------------
def test_checkpoint_roundtrip_of_a_uniform_agent(gpu, tmp_path):
    """tests/test_mlp_widths_gpu.py::test_checkpoint_roundtrip_at_width_128 for a uniform agent: every leaf back, an identical next
    update; an exp agent's state is refused with the message of a geometry mismatch and leaves the agent untouched"""
    from serl_amd.utils.checkpoint import read_checkpoint_tree, restore_checkpoint, save_checkpoint
    S, A, B = 10, 5, 8
    pk = PM.policy_kwargs("uniform", True)
    agent = MW.sac_agent(128, seed=7, B=B, S=S, A=A, policy_kwargs=pk)
    assert not agent.core.get("params", "actor/log_stds").any()      # zeros at init
    for i in range(2):
        agent.update_high_utd(_flat_batch(S, A, B, 10 + i), utd_ratio=2)
    assert agent.core.get("params", "actor/log_stds").all() and agent.core.get("opt/actor/mu", "actor/log_stds").all()
    save_checkpoint(str(tmp_path / "uniform"), agent, step=agent.state.step)
    tree = read_checkpoint_tree(str(tmp_path / "uniform"))
    assert tree["params"]["modules_actor"]["log_stds"].shape == (A,) and "Dense_1" not in tree["params"]["modules_actor"]
    assert np.array_equal(tree["params"]["modules_actor"]["log_stds"], agent.core.get("params", "actor/log_stds"))
    fresh = MW.sac_agent(128, seed=1, B=B, S=S, A=A, policy_kwargs=pk)
    restore_checkpoint(str(tmp_path / "uniform"), fresh, restore_rng=True)
    assert fresh.state.step == agent.state.step
    want = _all_bits(agent)
    assert ("params", "actor/log_stds") in want
    for key, v in _all_bits(fresh).items():
        assert _bits_equal(v, want[key]), key
    nxt = _flat_batch(S, A, B, 20)
    agent.update_high_utd(nxt, utd_ratio=1)
    fresh.update_high_utd(nxt, utd_ratio=1)
    want = _all_bits(agent)
    for key, v in _all_bits(fresh).items():
        assert _bits_equal(v, want[key]), ("after the next update", key)
    # an exp agent's state into the uniform agent, and the other way round
    other = MW.sac_agent(128, seed=7, B=B, S=S, A=A)
    other.update_high_utd(_flat_batch(S, A, B, 10), utd_ratio=2)
    save_checkpoint(str(tmp_path / "exp"), other, step=other.state.step)
    for target, path, leaf in ((fresh, "exp", "actor/log_stds"), (other, "uniform", "actor/logstd/kernel")):
        before, step_before = _all_bits(target), target.state.step
        with pytest.raises(ValueError, match=rf"leaf '{leaf}' has \d+ elements in this agent, the state holds 0 .*nothing was loaded"):
            restore_checkpoint(str(tmp_path / path), target)
        assert target.state.step == step_before
        for key, v in _all_bits(target).items():
            assert _bits_equal(v, before[key]), ("touched by the refused restore", key)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def _create(std_param=None, no_tanh=0):
    """serl_agent_create (std_param None) or serl_agent_create_policy of a state-only agent -> (status, serl_last_error(), leaf names)"""
    from serl_amd import _lib
    from serl_amd._lib_agent import SerlAgentCfg
    L = _lib.lib()
    cfg = SerlAgentCfg(0, 0, 0, 0, 10, 4, 8, 10, 256, 256, 8, 64, 0, -1, 0.99, 0.005, 3e-4, 0.1, 1e-5, 5.0, -2.0, 0)
    assert SerlAgentCfg._fields_[-1][0] == "num_stack"      # the struct is the one it was: the distribution is no field of it
    h = C.c_void_p()
    if std_param is None:
        rc = int(L.serl_agent_create(C.byref(cfg), C.byref(h)))
    else:
        rc = int(L.serl_agent_create_policy(C.byref(cfg), std_param, no_tanh, C.byref(h)))
    msg = (L.serl_last_error() or b"").decode()
    names = []
    if rc == 0:
        buf, cnt = C.create_string_buffer(128), C.c_int64()
        for i in range(L.serl_agent_num_leaves(h)):
            assert L.serl_agent_leaf_info(h, i, buf, 128, C.byref(cnt)) == 0
            names.append(buf.value.decode())
        assert int(L.serl_agent_destroy(h)) == 0
    return rc, msg, names


def test_c_abi_policy_fields(gpu):
    SERL_ERR_INVALID = -1      # include/serl_mi355.h
    before = list(O.trainable_param_shapes(O.Config(image_keys=(), S=10, A=4)))
    rc, msg, names = _create()
    assert rc == 0 and names == before, (rc, msg, names)          # serl_agent_create builds the agent it always did
    rc, msg, _ = _create(std_param=3)
    assert rc == SERL_ERR_INVALID and "std_param 3" in msg, (rc, msg)
    rc, msg, _ = _create(std_param=-1)
    assert rc == SERL_ERR_INVALID and "std_param -1" in msg, (rc, msg)
    rc, msg, _ = _create(0, no_tanh=2)
    assert rc == SERL_ERR_INVALID and "no_tanh 2" in msg, (rc, msg)
    for std_param in (0, 1, 2):
        for no_tanh in (0, 1):
            rc, msg, names = _create(std_param, no_tanh)
            assert rc == 0, (std_param, no_tanh, rc, msg)
            want = before if std_param != 2 else [n for n in before if "logstd" not in n][:-1] + ["actor/log_stds", "temp/lagrange"]
            assert names == want, (std_param, no_tanh, names)
