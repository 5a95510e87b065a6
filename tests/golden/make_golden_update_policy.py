"""Generates the policy-distribution fixtures: the REFERENCE's own SACAgent / DrQAgent (serl_launcher/agents/continuous/{sac,drq}.py,
networks/actor_critic_nets.py:167-227), imported unmodified from its checkout and run under the stand-ins of oracle/jaxshim in fp64,
with a policy distribution other than the launcher's ("exp" + tanh).  Run in the build container (needs the reference):
    python tests/golden/make_golden_update_policy.py [name ...]

The launcher factories write their own policy_kwargs into create_states / create_drq (utils/launcher.py:50-116), so the two create
functions are wrapped AT RUN TIME, as make_golden_update_widths.py wraps them for hidden_dims: the wrapper overrides
std_parameterization / tanh_squash_distribution in the `policy_kwargs` the factory passes.  The run itself is given the launcher's
Config (its recipes start from the launcher's leaves, and that is the cfg record of the files); the run's leaf table
(oracle.ref_update_runner.theta_flax_paths, looked up at run time) is the one of the mode's Config: for "uniform" no
modules_actor/Dense_1, and ("modules_actor", "log_stds") instead.

  policy_update_sac_state_{softplus,gauss,uniform,uniform_gauss}.npz   S = 10, A = 5, 72 rows; high_utd 2, update, high_utd 1
  policy_update_drq_uniform.npz                                        one camera 64x64, S = 5, A = 3, 6 rows; critics, high_utd 2
  policy_trained_sac_state_{softplus,uniform}.npz                      the state-only schedule from policy_modes.mode_theta's
      "trained" leaves: one std column below std_min in every row, one above std_max in every row, the rest inside

Every file records under meta["policy"] the distribution, the regime and what the reference's parameter tree holds in place of the
log-std leaves.  For the trained files, SACAgent.forward_policy is wrapped to read `.stddev()` of every distribution the update code
builds: per evaluation and action column the fraction of rows clipped low / high is asserted (at least one column low in all rows,
one high in all rows, two unclipped in all rows) and stored as policy_clip_low / policy_clip_high [evaluation][A].

The file names do not start with "update_": tests/test_reference_update.py and tests/test_golden_update_gpu.py run every
update_*.npz through the launcher's distribution.  tests/test_policy_modes_{cpu,gpu}.py read these files.
"""
import contextlib
import dataclasses
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from oracle import drq_oracle as O  # noqa: E402
from oracle import ref_update_runner as RR  # noqa: E402
import golden_replay as GR  # noqa: E402
import policy_modes as PM  # noqa: E402
import variant_recorder as VR  # noqa: E402

ONLY = [a for a in sys.argv[1:] if not a.startswith("-")]


@contextlib.contextmanager
def reference_policy(cfg, std, squash, stddevs):
    """create_states / create_drq with this distribution, the run's leaf table for it, and every forward_policy's stddev recorded"""
    with VR.reference_create_overrides({"policy_kwargs": {"std_parameterization": std, "tanh_squash_distribution": squash}}):
        from jax._core import raw
        from serl_launcher.agents.continuous.sac import SACAgent
        fp = SACAgent.__dict__["forward_policy"]

        def forward_policy(self, *a, _orig=fp, **k):
            dist = _orig(self, *a, **k)
            base = dist.distribution if squash else dist     # (the tanh distribution's own stddev() is tanh of the Gaussian's)
            stddevs.append(np.asarray(raw(base.stddev()).detach().cpu().numpy(), np.float64))
            return dist
        SACAgent.forward_policy = forward_policy
        paths = RR.theta_flax_paths
        RR.theta_flax_paths = lambda c: paths(cfg)
        try:
            yield
        finally:
            RR.theta_flax_paths, SACAgent.forward_policy = paths, fp


def check_tree(tree, std):
    """the mode took effect: the reference's own parameter tree says so -> what it holds behind the mean head"""
    actor = tree["modules_actor"]
    if std == "uniform":
        assert "log_stds" in actor and "Dense_1" not in actor, sorted(actor)
        assert tuple(actor["log_stds"]) == tuple(actor["Dense_0"]["bias"]), actor["log_stds"]
        return "log_stds"
    assert "Dense_1" in actor and "log_stds" not in actor, sorted(actor)
    return "Dense_1"


def clip_fractions(cfg, stddevs):
    """-> (low, high) [evaluation][A]: fraction of rows whose std sits on std_min / std_max; asserts the fixture's condition"""
    low = np.stack([(s == cfg.std_min).mean(axis=0) for s in stddevs])
    high = np.stack([(s == cfg.std_max).mean(axis=0) for s in stddevs])
    for i, (lo, hi) in enumerate(zip(low, high)):
        assert (lo == 1.0).sum() >= 1, ("no column clipped low in all rows", i, lo)
        assert (hi == 1.0).sum() >= 1, ("no column clipped high in all rows", i, hi)
        assert ((lo == 0.0) & (hi == 0.0)).sum() >= 2, ("fewer than two columns unclipped in all rows", i, lo, hi)
    return low, high


def main():
    for name, (cfg, B, sched, (std, squash), regime, n_sample) in PM.GOLDEN.items():
        if ONLY and name not in ONLY:
            continue
        os.environ.pop("SERL_JAXSHIM_PRNG", None)
        stddevs = []
        with reference_policy(cfg, std, squash, stddevs):
            res = RR.run_reference(dataclasses.replace(cfg, std_parameterization="exp", tanh_squash=True), B, sched, GR.PARAM_SEED,
                                   GR.BATCH_SEED, theta_transform=lambda th, c: PM.mode_theta(th, c, std, regime))
        holds = check_tree(res["final"]["param_tree"], std)
        assert (cfg.std_parameterization, cfg.tanh_squash) == (std, squash)
        assert set(res["final"]["params"]) == set(O.trainable_param_shapes(cfg))
        assert stddevs and all(s.shape[-1] == cfg.A for s in stddevs)
        meta = {"std_parameterization": std, "tanh_squash_distribution": squash, "regime": regime, "std_leaves": holds,
                "transform": "policy_modes.mode_theta", "log_stds_seed": PM.LOG_STDS_SEED, "clip_cycle": list(PM.CLIP_CYCLE),
                "policy_evaluations": len(stddevs)}
        extra = dict(zip(("policy_clip_low", "policy_clip_high"), clip_fractions(cfg, stddevs))) if regime == "trained" else None
        VR.write(GR.variant_path("policy", name), res, GR.PARAM_SEED, GR.BATCH_SEED, n_sample_key="policy_n_sample", n_sample=n_sample,
                 meta_key="policy", meta=meta, extra=extra)


if __name__ == "__main__":
    main()
