"""CPU: the restatement of the read-only evaluation (tests/eval_oracle.py) against the reference's own answers, and the resources
of the kernel that serves it.

  * tests/golden/eval_*.npz hold what the reference's SACAgent / DrQAgent answered to forward_critic(train=False), the same with
    target_params, and forward_policy(train=False).distribution.loc / .scale_diag / .mode() / .log_prob(actions)
    (tests/golden/make_golden_eval.py).  The fp64 restatement reproduces all six quantities with the bound of
    tests/test_reference_update.py (1e-9 relative to the leaf's scale, oracle.golden_update.leaf_compare).
  * Its fp32 run against its fp64 run gives the yardstick of log_prob per case, under the per-row measure the GPU test uses
    (|error| / max(1, |reference|), worst row).  Measured: sac_state 1.3e-7, drq_one_cam 2.0e-7, sac_state_softplus_gauss 1.6e-7,
    sac_state_uniform 1.5e-7 -- the clipped std_min column puts |log_prob| near 1e12 and the measure is then relative.
  * heads.hip compiled for gfx950 with the compiler's resource remarks (no link, no GPU): every policy_stats_kernel instantiation
    allocates at most 80 registers -- the chain budget of scripts/kernel_resources.py, what two resident trunk workgroups leave --
    and uses no scratch and no LDS (it is launched without dynamic LDS).  Measured: 13 to 40 registers
    (allocation 16 to 40) over the six modes, scratch 0, LDS 0."""
import dataclasses
import json
import os
import shutil
import sys

import numpy as np
import pytest
import torch

from oracle import golden_update as G
import eval_oracle as EO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
F64_TOL = 1e-9      # tests/test_reference_update.py


def _golden(name):
    z = np.load(EO.golden_path(name))
    meta = json.loads(str(z["meta"]))
    return meta, {q: {"full": z[f"{q}/full"]} for q in EO.QUANTITIES}


_RESTATED = {}


def restated(name):
    """-> (fp64 results, fp32 log_prob error) of a fixture's case; computed once per session"""
    if name not in _RESTATED:
        cfg, B, _ = EO.GOLDEN[name]
        trunk, theta, target = EO.leaves(cfg)
        pb = EO.golden_inputs(name)
        frames = {k: v[:, 0] for k, v in pb["frames"].items()}
        _RESTATED[name] = EO.log_prob_yardstick(cfg, trunk, theta, target, frames, pb["state"][:, 0], pb["action"])
    return _RESTATED[name]


@pytest.mark.parametrize("name", sorted(EO.GOLDEN))
def test_the_restatement_reproduces_the_reference(name):
    meta, rec = _golden(name)
    cfg, B, (std, squash) = EO.GOLDEN[name]
    assert meta["B"] == B and meta["std_parameterization"] == std and meta["tanh_squash_distribution"] == squash
    assert (cfg.std_parameterization, cfg.tanh_squash) == (std, squash)
    assert dataclasses.replace(G.cfg_from_dict(meta["cfg"]), std_parameterization=std, tanh_squash=squash) == cfg      # (the file's cfg record is the launcher's)
    assert meta["batch_seed"] == EO.BATCH_SEED
    r64, _ = restated(name)
    assert np.abs(EO.golden_inputs(name)["action"]).max() <= EO.ACTION_BOUND
    for q in EO.QUANTITIES:
        assert list(r64[q].shape) == meta["shapes"][q], (q, r64[q].shape)
        e, how = G.leaf_compare(q, rec[q], r64[q])
        print(name, q, e)
        assert e < F64_TOL, (q, how, e)
    assert np.abs(rec["q"]["full"] - rec["q_target"]["full"]).max() > 1e-3      # the target copy differs


@pytest.mark.parametrize("name", sorted(EO.GOLDEN))
def test_log_prob_yardstick_of_the_fp32_restatement(name):
    r64, err32 = restated(name)
    print(name, "fp32 restatement, log_prob:", err32)
    assert np.isfinite(r64["log_prob"]).all()
    # fp32 arithmetic on a sum of A terms, measured relative: a few units of 2^-24 per operation, far from the GPU test's floor
    assert 0.0 < err32 < 1e-5, err32


def test_a_stored_action_at_the_bound_is_not_finite():
    cfg, B, _ = EO.GOLDEN["sac_state"]
    trunk, theta, target = EO.leaves(cfg)
    pb = EO.golden_inputs("sac_state")
    a = pb["action"].copy()
    a[1, 2], a[4, 0] = 1.0, -1.0
    r = EO.evaluate(cfg, trunk, theta, target, {}, pb["state"][:, 0], a, torch.float64)
    bad = ~np.isfinite(r["log_prob"])
    assert bad.tolist() == [i in (1, 4) for i in range(B)]


def test_policy_stats_kernel_fits_the_chain_budget_without_scratch_or_lds():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc is not installed")
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources as KR
    raw = KR.remarks(HIPCC, "heads.hip")
    short = KR.demangle(list(raw))
    mine = {short[n]: v for n, v in raw.items() if short[n].startswith("policy_stats_kernel<")}
    assert len(mine) == 6, sorted(mine)        # the six std parameterisation x squash modes
    for name, v in sorted(mine.items()):
        regs = int(v["VGPRs"]) + int(v["AGPRs"])
        alloc = (regs + 7) // 8 * 8            # the allocation granule of scripts/kernel_resources.py
        print(name, "registers", regs, "allocation", alloc, "scratch", v["ScratchSize [bytes/lane]"], "LDS", v["LDS Size [bytes/block]"])
        assert alloc <= 80, (name, v)
        assert int(v["ScratchSize [bytes/lane]"]) == 0 and int(v["LDS Size [bytes/block]"]) == 0, (name, v)
    assert any(b == 80 for n, b in KR.CHAIN if n.startswith("policy_stats_kernel<")), "the kernel is on the chain budget list"
