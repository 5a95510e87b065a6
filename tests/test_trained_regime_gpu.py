"""GPU: the SAC/DrQ update chain of serl_amd/csrc/heads.hip + agent.hip AWAY from O.init_params -- the regime of a trained policy
(tests/trained_regime.py, its conditions proved in tests/test_trained_regime_cpu.py): exp(log_std) clipped at std_min and at
std_max in whole columns, tanh saturated to exactly +-1, exp(2|u|) beyond the fp32 range in one case, |Q| of tens, alpha from 2.5e-3
to 4, masks all zero / all one / mixed, rewards of both signs, stored actions at +-1, a target copy that differs from the online
parameters.  Every other parity test of the chain starts from O.init_params, where log_std stays in [-3, 1.9]: std_max binds in a
few percent of the entries of some cases and std_min never, |u| stays below 3 and |Q| below 1.

* the HIP chain (fused and SERL_CHAIN_FUSE=0) against the fp64 oracle after update_critics, update_high_utd(1) and one UTD > 1:
  info scalars, the q / target_q / logp taps, every gradient leaf, the state and the step counters at TOL = 1e-4 of
  tests/test_agent_gpu.py;
* exact zeros: the clipped columns of the log_std head's gradients are 0.0 and their parameters and actor moments do not move;
* the policy head's gradients column by column, each normalised by its own maximum, within max(1e-4, 4 x the float32 oracle's
  error under the same measure) -- AH.rel_err per leaf lets a strong column hide a weak one;
* the fused chain against the one-launch-per-operation chain bit for bit with a binding clip;
* sample_actions (mode and injected eps) within 1e-5 absolute, finite and inside [-1, 1];
* the reference's own update code in the regime (tests/golden/trained_update_*.npz) with the comparisons and bounds of
  tests/test_golden_update_gpu.py.

Measured on an MI355X, worst over all cases and both chains: info scalars 5.4e-06, taps 2.8e-07, gradient leaves 2.0e-06, state
(99.9th percentile) 9.2e-06; policy-head columns 8.9e-06 (float32 oracle 2.0e-06, at most 0.09 of the bound); sample_actions
1.4e-07; against the goldens: Adam moments 1.5e-05, parameters 1.1e-05."""
import numpy as np
import pytest
import torch

from oracle import drq_oracle as O
import agent_helpers as AH
import golden_replay as GR
import trained_regime as TR
from test_agent_gpu import TOL, _check_grads, _compare_state
from test_chain_fusion_gpu import _assert_state_bits, _bits_equal

pytestmark = pytest.mark.gpu
FUSE = [pytest.param(True, id="fused"), pytest.param(False, id="unfused")]
CRITIC_INFO = ("critic_loss", "predicted_qs", "target_qs")
ALL_INFO = CRITIC_INFO + ("actor_loss", "temperature", "entropy", "temperature_loss")


def _core(case, lam, fuse):
    _, cfg, B, _, cyc = case
    return TR.pair(cfg, B, lam, fuse=fuse, mean_cycle=cyc)[1]


def _infos(what, got, ref, names):
    bad = []
    for k in names:
        e = abs(got[k] - ref[k]) / max(1.0, abs(ref[k]))
        print(f"{what}: info {k} = {got[k]:.6g} (oracle {ref[k]:.6g}), err {e:.2e}")
        if not e < TOL:
            bad.append((k, got[k], ref[k], e))
    assert not bad, (what, bad)


def _grads(what, cfg, core, grads, tap, lo0):
    """prints the worst leaf of the tap, then tests/test_agent_gpu.py::_check_grads (every leaf < TOL)"""
    sl, _ = AH.leaf_slices(cfg)
    hi = sl.get("enc/proprio/ln/bias", sl["critic/head/bias"])[1] if tap == "g_critic" else sl["actor/logstd/bias"][1]
    g = core.debug(tap, hi - lo0)
    errs = {k: AH.rel_err(g[sl[k][0] - lo0:sl[k][1] - lo0], gv.numpy().reshape(-1)) for k, gv in grads.items()}
    k = max(errs, key=errs.get)
    print(f"{what}: {tap} worst leaf {k} = {errs[k]:.2e}")
    _check_grads(cfg, core, grads, tap, lo0)


def _actor_lo(cfg):
    sl, _ = AH.leaf_slices(cfg)
    return sl, sl.get("enc/proprio/dense/kernel", sl["actor/w1"])[0]


def _actor_grad(cfg, core):
    """-> {leaf: flat gradient} of the actor optimizer's support, from the g_actor tap"""
    sl, lo0 = _actor_lo(cfg)
    g = core.debug("g_actor", sl["actor/logstd/bias"][1] - lo0)
    return {k: g[sl[k][0] - lo0:sl[k][1] - lo0] for k in TR.POLICY_HEAD_LEAVES}


def _clipped(cfg):
    low, _, high = TR.clip_columns(cfg)
    return np.concatenate([low, high])


def _assert_exact_zeros(what, cfg, core, lam, cyc):
    """the kernel writes 0.f where the clip binds and sums of zeros are zeros: no tolerance"""
    g, cols = _actor_grad(cfg, core), _clipped(cfg)
    assert (g["actor/logstd/bias"][cols] == 0.0).all(), (what, g["actor/logstd/bias"])
    assert (g["actor/logstd/kernel"].reshape(-1, cfg.A)[:, cols] == 0.0).all(), what
    _, theta, _ = TR.theta_pair(cfg, lam, cyc)
    for leaf in ("actor/logstd/kernel", "actor/logstd/bias"):
        before = np.asarray(theta[leaf], np.float32).reshape(-1, cfg.A)[:, cols]
        assert _bits_equal(core.get("params", leaf).reshape(-1, cfg.A)[:, cols], before), (what, "params moved", leaf)
        assert _bits_equal(core.get("opt/actor/mu", leaf).reshape(-1, cfg.A)[:, cols], np.zeros_like(before)), (what, "mu", leaf)


def _assert_columns(what, cfg, core, r64, r32):
    g, bad, worst = _actor_grad(cfg, core), [], 0.0
    for k in TR.POLICY_HEAD_LEAVES:
        ref = r64["aux2"]["g_actor"][k].numpy()
        e = TR.column_errors(cfg, g[k], ref)
        y = TR.column_errors(cfg, r32["aux2"]["g_actor"][k].numpy(), ref)
        for j in range(cfg.A):
            if np.isnan(y[j]):       # an exactly-zero reference column: _assert_exact_zeros
                continue
            bound = max(TOL, 4.0 * y[j])
            worst = max(worst, e[j] / bound)
            print(f"{what}: {k} column {j}: err {e[j]:.2e}, float32 oracle {y[j]:.2e}, err / bound {e[j] / bound:.2f}")
            if not e[j] <= bound:
                bad.append((k, j, e[j], y[j]))
    assert not bad, (what, bad)
    return worst


@pytest.mark.parametrize("fuse", FUSE)
@pytest.mark.parametrize("case,lam,mode", TR.RUNS, ids=TR.RUN_IDS)
def test_update_chain_matches_the_oracle_in_the_regime(gpu, case, lam, mode, fuse):
    """update_critics, then update_high_utd(1).  Measured on an MI355X: worst policy-head column 8.9e-06 of its own maximum, where the
    float32 oracle measures 2.0e-06: err / bound at most 0.09; worst gradient leaf 2.0e-06, worst info scalar 5.4e-06"""
    name, cfg, B, _, cyc = case
    what = f"{name} lam {lam:g} {mode} {'fused' if fuse else 'unfused'}"
    r64, r32 = TR.reference_run(case, lam, mode), TR.reference_run(case, lam, mode, torch.float32)
    core = _core(case, lam, fuse)
    b1, n1, b2, n2 = TR.inputs(case, mode)
    core.update_critics(AH.batch_to_device(cfg, b1), AH.noise_to_device(cfg, n1))
    _infos(what + " update_critics", core.read_info(), r64["info1"], CRITIC_INFO)
    aux = r64["aux1"]
    taps = {"q": AH.rel_err(core.debug("q", cfg.ensemble * B).reshape(cfg.ensemble, B), aux["q"].numpy()),
            "target_q": AH.rel_err(core.debug("target_q", B), aux["target_q"].numpy()),
            "logp": AH.rel_err(core.debug("logp", B), aux["next_logp"].numpy())}
    print(f"{what}: taps {({k: f'{v:.2e}' for k, v in taps.items()})}")
    assert all(v < TOL for v in taps.values()), (what, taps)
    assert np.isfinite(core.debug("logp", B)).all()
    _grads(what, cfg, core, aux["grads"], "g_critic", 0)
    print(f"{what}: state after update_critics (99.9 pct) = {_compare_state(cfg, r64['after1'], core):.2e}")
    assert core.step == r64["after1"].step == 1
    core.update_high_utd(AH.batch_to_device(cfg, b2), 1, AH.noise_to_device(cfg, n2))
    _infos(what + " update_high_utd(1)", core.read_info(), r64["info2"], ALL_INFO)
    _grads(what, cfg, core, r64["aux2"]["g_actor"], "g_actor", _actor_lo(cfg)[1])
    _assert_exact_zeros(what, cfg, core, lam, cyc)
    worst = _assert_columns(what, cfg, core, r64, r32)
    print(f"{what}: worst policy-head column err / bound = {worst:.2f}")
    print(f"{what}: state after update_high_utd(1) (99.9 pct) = {_compare_state(cfg, r64['after2'], core, steps=3):.2e}")
    assert core.step == r64["after2"].step == 3
    assert core.debug("ctr_nonzero", 1)[0] == 0


@pytest.mark.parametrize("fuse", FUSE)
@pytest.mark.parametrize("case,lam,mode", TR.RUNS, ids=TR.RUN_IDS)
def test_update_high_utd_above_one_matches_the_oracle_in_the_regime(gpu, case, lam, mode, fuse):
    """UTD = 2, or the smallest divisor of an odd row count (sac.py:561-563 refuses a batch the ratio does not divide)"""
    name, cfg, B, _, cyc = case
    utd = TR.second_utd(B)
    what = f"{name} lam {lam:g} {mode} {'fused' if fuse else 'unfused'} update_high_utd({utd})"
    r = TR.reference_run_utd(case, lam, mode, utd)
    core = _core(case, lam, fuse)
    _, _, b2, n2 = TR.inputs(case, mode, utd)
    core.update_high_utd(AH.batch_to_device(cfg, b2), utd, AH.noise_to_device(cfg, n2))
    _infos(what, core.read_info(), r["info"], ALL_INFO)
    _grads(what, cfg, core, r["aux"]["g_actor"], "g_actor", _actor_lo(cfg)[1])
    _assert_exact_zeros(what, cfg, core, lam, cyc)
    print(f"{what}: state (99.9 pct) = {_compare_state(cfg, r['after'], core, steps=utd + 1):.2e}")
    assert core.step == r["after"].step == utd + 1
    assert core.debug("ctr_nonzero", 1)[0] == 0


@pytest.mark.parametrize("case,lam,mode", TR.RUNS, ids=TR.RUN_IDS)
def test_fused_chain_is_bit_identical_to_the_unfused_chain_in_the_regime(gpu, case, lam, mode):
    """the taps of tests/test_chain_fusion_gpu.py, with a binding clip"""
    name, cfg, B, _, cyc = case
    fused, plain = _core(case, lam, True), _core(case, lam, False)
    sl, pa0 = _actor_lo(cfg)
    pc, pa1 = sl.get("enc/proprio/ln/bias", sl["critic/head/bias"])[1], sl["actor/logstd/bias"][1]
    b1, n1, b2, n2 = TR.inputs(case, mode)
    for core in (fused, plain):
        core.update_critics(AH.batch_to_device(cfg, b1), AH.noise_to_device(cfg, n1))
        core.update_high_utd(AH.batch_to_device(cfg, b2), 1, AH.noise_to_device(cfg, n2))
    for tap, n in (("g_critic", pc), ("g_actor", pa1 - pa0), ("scalars", 8), ("q", cfg.ensemble * B), ("target_q", B), ("logp", B),
                   ("dx", B * (cfg.enc_dim + cfg.A))):
        assert _bits_equal(fused.debug(tap, n), plain.debug(tap, n)), (name, lam, mode, tap)
    fi, pi = fused.read_info(), plain.read_info()
    assert fi == pi, (name, lam, mode, fi, pi)
    _assert_state_bits(cfg, fused, plain, (name, lam, mode))


@pytest.mark.parametrize("case", TR.CASES, ids=[c[0] for c in TR.CASES])
def test_sample_actions_match_the_oracle_in_the_regime(gpu, case):
    name, cfg, B, modes, cyc = case
    lam = modes[0][0]
    st, core = TR.pair(cfg, B, lam, mean_cycle=cyc)
    b = AH.synth_batch(cfg, B, seed=6)
    frames = torch.tensor(np.stack([b["obs"][k] for k in cfg.image_keys]), device="cuda") if cfg.image_keys else None
    state = torch.tensor(b["state"], device="cuda")
    feats = O.features(st, {k: torch.tensor(v) for k, v in b["obs"].items()})
    enc = O.encode(st.params, cfg, feats, torch.tensor(b["state"], dtype=torch.float64))
    mean, std = O.policy_head(st.params, cfg, enc)
    low, _, high = TR.clip_columns(cfg)
    assert (std[:, low] == cfg.std_min).all() and (std[:, high] == cfg.std_max).all()
    eps = np.random.default_rng(0).standard_normal((B, cfg.A)).astype(np.float32)
    want = {"mode": torch.tanh(mean).numpy(), "sample": torch.tanh(mean + std * torch.tensor(eps, dtype=torch.float64)).numpy()}
    got = {"mode": core.sample_actions(frames, state, None).cpu().numpy(),
           "sample": core.sample_actions(frames, state, torch.tensor(eps, device="cuda")).cpu().numpy()}
    for k in want:
        err = float(np.abs(got[k].astype(np.float64) - want[k]).max())
        print(f"sample_actions {name}: {k} max abs err = {err:.2e}, |a| == 1 in {(np.abs(got[k]) == 1).mean():.0%}")
        assert np.isfinite(got[k]).all() and (np.abs(got[k]) <= 1.0).all(), (name, k)
        assert err <= 1e-5, (name, k, err)
    assert core.debug("ctr_nonzero", 1)[0] == 0


@pytest.mark.parametrize("name", TR.UPDATE_GOLDEN)
def test_hip_update_matches_the_reference_golden_in_the_regime(gpu, name):
    """tests/test_golden_update_gpu.py::test_hip_update_matches_the_reference_golden on trained_update_<name>.npz (injected noise)"""
    g, theta, target, trunk = TR.update_golden(name)
    agent = GR.reference_agent(g["cfg"], g["B"])
    AH.load_leaves(agent.core, g["cfg"], trunk, theta, target)
    GR.replay(agent, g, label=f"trained_update_{name}")
    assert agent.core.debug("ctr_nonzero", 1)[0] == 0
