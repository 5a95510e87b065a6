"""CPU: the trained regime of tests/trained_regime.py, proved on the oracle alone.

* For every case and mode the fp64 oracle shows what the recipe is for: policy columns clipped low, clipped high and unclipped in
  every row, log_std at least 0.5 away from both clip bounds (fp32 and fp64 decide the clip identically), saturated and unsaturated
  pre-tanh values, |Q| of tens, and a log_std bias gradient that is exactly zero in the clipped columns.  These are conditions on
  the inputs of tests/test_trained_regime_gpu.py, not measurements of the code under test.
* The same schedule in a float32 oracle state stays within 2e-5 of fp64 (measured: infos <= 5.3e-6, gradient leaves <= 1.3e-6, policy-head
  columns <= 2.2e-6; the figures are printed): a correct fp32 implementation attains the GPU tests' 1e-4 in this regime.
* tests/golden/trained_update_*.npz (tests/golden/make_golden_update_trained.py: the reference's own sac.py / actor_critic_nets.py
  on these parameters and batches) are reproduced by the oracle at the bound of tests/test_reference_update.py."""
import math

import numpy as np
import pytest
import torch

from oracle import drq_oracle as O
from oracle import golden_update as G
from oracle import ref_update_runner as RR
import agent_helpers as AH
import trained_regime as TR
from test_reference_update import F64_TOL, _oracle_sections

F32_YARDSTICK = 2e-5


@pytest.mark.parametrize("case,lam,mode", TR.RUNS, ids=TR.RUN_IDS)
def test_the_recipe_reaches_the_regime(case, lam, mode):
    name, cfg, B, _, cyc = case
    assert cfg.A >= 4
    r = TR.reference_run(case, lam, mode)
    lo_b, hi_b = math.log(cfg.std_min), math.log(cfg.std_max)
    low, mid, high = TR.clip_columns(cfg)
    us, margin = [], math.inf
    for ev, (mean, ls, eps) in r["pre"].items():
        ls, mean, eps = ls.numpy(), mean.numpy(), eps.numpy()
        assert ls.shape == (B, cfg.A)
        assert any((ls[:, j] < lo_b).all() for j in range(cfg.A)), (ev, "no column clipped low in every row")
        assert any((ls[:, j] > hi_b).all() for j in range(cfg.A)), (ev, "no column clipped high in every row")
        assert any(((ls[:, j] > lo_b) & (ls[:, j] < hi_b)).all() for j in range(cfg.A)), (ev, "no unclipped column")
        assert (ls[:, low] < lo_b).all() and (ls[:, high] > hi_b).all() and ((ls[:, mid] > lo_b) & (ls[:, mid] < hi_b)).all(), ev
        margin = min(margin, float(np.abs(ls - lo_b).min()), float(np.abs(ls - hi_b).min()))
        us.append(np.abs(mean + np.clip(np.exp(ls), cfg.std_min, cfg.std_max) * eps))
    u = np.concatenate([x.reshape(-1) for x in us])
    q_abs = float(r["aux1"]["q"].abs().mean())
    print(f"{name} lam {lam:g} {mode}: min |log_std - log(bound)| = {margin:.2f}, |u| > 9: {(u > 9).mean():.1%}, |u| < 2: {(u < 2).mean():.1%}, "
          f"max |u| = {u.max():.1f}, mean |Q| = {q_abs:.1f}, alpha = {r['info2']['temperature']:.3g}")
    assert margin >= 0.5, margin
    assert (u > 9).mean() >= 0.10 and (u < 2).mean() >= 0.20
    if cyc is TR.MEAN_CYCLE_OVERFLOW:
        assert u.max() >= 50
    assert q_abs >= 10
    g = r["aux2"]["g_actor"]["actor/logstd/bias"].numpy()
    assert (g[low] == 0.0).all() and (g[high] == 0.0).all(), g
    assert (g[mid] != 0.0).all(), g
    gk = r["aux2"]["g_actor"]["actor/logstd/kernel"].numpy()
    assert (gk[:, low] == 0.0).all() and (gk[:, high] == 0.0).all()
    # the batch is what harden_batch promises
    b1, _, b2, _ = TR.inputs(case, mode)
    for b in (b1, b2):
        assert (np.abs(b["action"][::4]) == 1.0).all() and np.abs(b["reward"]).max() > 20
        assert b["mask"].mean() == {"zero": 0.0, "one": 1.0}.get(mode, b["mask"].mean()) and (mode != "mixed" or 0 < b["mask"].mean() < 0.5)
    # the target copy differs from the online critic
    st = TR.oracle_state(cfg, lam, torch.float64, cyc)
    assert not torch.equal(st.target["critic/w2"], st.params["critic/w2"]) and not torch.equal(st.target["critic/head/bias"], st.params["critic/head/bias"])


@pytest.mark.parametrize("case,lam,mode", TR.RUNS, ids=TR.RUN_IDS)
def test_plain_fp32_attains_the_bound_in_the_regime(case, lam, mode):
    """the yardstick: oracle in float32 against the oracle in float64, same schedule, same measures as the GPU test"""
    name, cfg = case[0], case[1]
    r64, r32 = TR.reference_run(case, lam, mode), TR.reference_run(case, lam, mode, torch.float32)
    worst_i = worst_g = 0.0
    for ki in ("info1", "info2"):
        for k, ref in r64[ki].items():
            worst_i = max(worst_i, abs(r32[ki][k] - ref) / max(1.0, abs(ref)))
    for aux, gk in (("aux1", "grads"), ("aux2", "g_actor")):
        for k, ref in r64[aux][gk].items():
            worst_g = max(worst_g, AH.rel_err(r32[aux][gk][k].numpy(), ref.numpy()))
    worst_c = 0.0
    for k in TR.POLICY_HEAD_LEAVES:
        worst_c = max(worst_c, float(np.nanmax(TR.column_errors(cfg, r32["aux2"]["g_actor"][k].numpy(), r64["aux2"]["g_actor"][k].numpy()))))
    print(f"{name} lam {lam:g} {mode}: fp32 oracle vs fp64: infos {worst_i:.1e}, gradient leaves {worst_g:.1e}, policy-head columns {worst_c:.1e}")
    assert worst_i <= F32_YARDSTICK and worst_g <= F32_YARDSTICK, (worst_i, worst_g)


def _run_oracle(g, theta, target, trunk):
    cfg = g["cfg"]
    st = O.TrainState(cfg, trunk, theta, torch.float64)
    st.target = O.to_torch(target, torch.float64)
    return st, RR.run_steps(st, g["steps"], torch.float64)


@pytest.mark.parametrize("name", TR.UPDATE_GOLDEN)
def test_oracle_reproduces_the_reference_golden_in_the_regime(name):
    """tests/test_reference_update.py::test_oracle_reproduces_the_reference_golden on trained_update_<name>.npz"""
    g, theta, target, trunk = TR.update_golden(name)
    cfg = g["cfg"]
    assert cfg.A >= 4 and [s["kind"] for s in g["steps"]] == ([("update" if cfg.state_only else "critics"), "high_utd", "update",
                                                               ("update" if cfg.state_only else "critics")])
    assert np.abs(g["steps"][0]["batch"]["reward"]).max() > 20
    st, infos = _run_oracle(g, theta, target, trunk)
    for i, (info, step) in enumerate(zip(infos, g["steps"])):
        for k, v in info.items():
            r = step["info"][k]
            assert abs(v - r) <= F64_TOL * max(1.0, abs(r)), (i, k, v, r)
    assert abs(g["steps"][0]["info"]["predicted_qs"]) >= 5      # the recorded run is in the regime
    assert st.step == g["meta"]["final_step"]
    worst = 0.0
    low, _, high = TR.clip_columns(cfg)
    for sec, tree in _oracle_sections(st).items():
        assert set(g["final"][sec]) == set(tree), sec
        for leaf, t in tree.items():
            e, how = G.leaf_compare(f"{sec}/{leaf}", g["final"][sec][leaf], t.numpy())
            assert e < F64_TOL, (sec, leaf, how, e)
            worst = max(worst, e)
    # the reference's own Adam moment of the clipped log_std columns is exactly zero
    mu = g["final"]["mu_actor"]["actor/logstd/bias"]["full"]
    assert (mu[low] == 0.0).all() and (mu[high] == 0.0).all() and (mu != 0.0).sum() == cfg.A - len(low) - len(high), mu
    print(f"trained_update_{name}: oracle vs reference golden, worst {worst:.1e}")
