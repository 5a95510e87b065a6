"""Shared by tests/test_wide_actions_{cpu,gpu}.py: action widths above 64 (wide_actions=True, serl_agent_opts.wide_actions; up to
256), the wide head rows of serl_amd/csrc/head_wide.h.  The case table, agent_helpers.make_core with the switch and the fp64 oracle
run of a case (tests/test_evaluate_gpu.py's leaves: "trained" puts whole std columns on both clips, as tests/policy_modes.py chooses
them; the fixed std as tests/policy_fixed.py states it: the oracle in "uniform" with actor/log_stds pinned)."""
import contextlib
import functools

import numpy as np
import torch

from oracle import drq_oracle as O
import agent_helpers as AH
import policy_fixed as PF
import policy_modes as PM
import test_evaluate_gpu as TE

# (A, rows): one live lane in the second block, exact blocks, a ragged fourth block, the cap; one row and one past a 64-row tile
UPDATES = {f"A{A}_B{B}": dict(A=A, B=B) for A in (65, 128, 200, 256) for B in (1, 65)}
MODES = {   # at A = 200, 65 rows
    "softplus_tanh": dict(A=200, B=65, std="softplus"),
    "uniform_tanh": dict(A=200, B=65, std="uniform"),
    "fixed_tanh_clipped_both_ways": dict(A=200, B=65, fixed=tuple(np.geomspace(0.02, 4.0, 200))),      # std_min 0.05, std_max 2
    "exp_gauss_backup_entropy": dict(A=200, B=65, squash=False, backup_entropy=True),
    "exp_tanh_clipped_columns": dict(A=200, B=65, regime="trained"),
    "small_32x32_A65": dict(A=65, B=5, pixels=True),      # the action columns behind 256 + 64 code columns of the critic's input
}
CASES = {**UPDATES, **MODES}
BC_CASE = ("one_cam_B65_A200", ("wrist",), 32, 32, 65, 200)      # tests/image_only_bc.py's case form


def config(A, std="exp", squash=True, backup_entropy=False, pixels=False, fixed=None, **_):
    if fixed is not None:
        return PF.config("state", 10, A, fixed, ensemble=2, std_min=0.05, std_max=2.0, critic_dims=(64, 64), policy_dims=(64, 64), warmup=4, temp_warmup=0)
    img = dict(image_keys=("wrist",), H=32, W=32, encoder_type="small", S=5) if pixels else dict(image_keys=(), S=10)
    return PM.mode_config(std, squash, A=A, ensemble=2, discount=0.99, hidden=64, warmup=4, temp_warmup=0, backup_entropy=backup_entropy, **img)


def oracle_of(cfg):
    """the oracle a Config runs under: tests/policy_fixed.py's general one for a fixed std, the plain one else"""
    return PF.installed() if getattr(cfg, "fixed_std", None) is not None else contextlib.nullcontext()


def make_core(cfg, B, leaves=None, *, fuse=None, wide_actions=True, **kw):
    """agent_helpers.make_core with serl_agent_opts.wide_actions set (AgentCore's keyword, for the call); leaves: (trunk, theta, target)"""
    import serl_amd.agents.core as core_mod
    orig = core_mod.AgentCore
    core_mod.AgentCore = functools.partial(orig, wide_actions=wide_actions)
    try:
        core = AH.make_core(cfg, B, fuse=fuse, **kw)
    finally:
        core_mod.AgentCore = orig
    return core if leaves is None else AH.load_leaves(core, cfg, *leaves)


_RUNS = {}


def oracle_run(name, dtype=torch.float64):
    """one update_high_utd(1) -- critic, actor, temperature, Adam, EMA -- of the case in `dtype`: computed once, unchanged by its
    readers.  "state" is what _compare_state reads, "g_actor" the compared gradient leaves."""
    if (name, dtype) not in _RUNS:
        c = CASES[name]
        cfg, B = config(**c), c["B"]
        with oracle_of(cfg):
            fixed = getattr(cfg, "fixed_std", None) is not None
            trunk, theta, _ = (*PF.init_params(cfg, 42), None) if fixed else TE._leaves(cfg, c.get("regime", "init"))
            st = PF.pinned_state(cfg, trunk, theta, dtype) if fixed else O.TrainState(cfg, trunk, theta, dtype)
            b, noise = AH.synth_batch(st.cfg, B, seed=4), O.make_noise(st.cfg, B, seed=8, utd_ratio=1)
            with (PF.pinned(cfg) if fixed else contextlib.nullcontext()):
                info, aux = O.update_high_utd(st, AH.batch_to_torch(b, dtype), O.noise_to_torch(noise, dtype), 1)
        _RUNS[name, dtype] = dict(cfg=cfg, B=B, leaves=(trunk, theta, None), batch=b, noise=noise, info=info, logp=aux["logp"].numpy(),
                                  state=PF.compared_state(st) if fixed else st, g_actor=PF.unpinned(aux["g_actor"]))
    return _RUNS[name, dtype]
