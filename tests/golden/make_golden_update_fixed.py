"""Generates the fixed-std fixtures: the REFERENCE's own SACAgent / DrQAgent (serl_launcher/agents/continuous/{sac,drq}.py,
networks/actor_critic_nets.py:167-227), imported unmodified from its checkout and run under the stand-ins of oracle/jaxshim in fp64,
with policy_kwargs std_parameterization="fixed" and a fixed_std vector.  Run in the build container (needs the reference):
    python tests/golden/make_golden_update_fixed.py [name ...]

Built like make_golden_update_policy.py.  The launcher factories write their own policy_kwargs into create_states / create_drq
(utils/launcher.py:50-116), so the two create functions are wrapped AT RUN TIME (variant_recorder.reference_create_overrides) and
the wrapper overrides std_parameterization / fixed_std / tanh_squash_distribution / std_min / std_max in the `policy_kwargs` the
factory passes.  The run itself is given the launcher's Config (its recipe starts from the launcher's leaves, and that is the cfg
record of the files); the run's leaf table (oracle.ref_update_runner.theta_flax_paths, looked up at run time) is the "uniform" one
WITHOUT actor/log_stds: a fixed head has no std leaf.  fixed_std is a length-A vector in every file -- whether the real distrax
takes a 0-d scale_diag cannot be checked without it -- and its entries are float32 values, the ones the library holds.

  fixed_update_sac_state.npz        case (a) of tests/policy_fixed.py: S = 10, A = 5, 72 rows, two columns clipped;
                                    high_utd 2, update, high_utd 1
  fixed_update_sac_state_gauss.npz  case (b): tanh_squash_distribution=False, backup_entropy=True, with policy_fixed.GAUSS_VECTOR
  fixed_update_drq.npz              case (e): one camera 64x64, S = 5, A = 3, 6 rows; critics, high_utd 2

Asserted on the reference's own objects before a file is written: its modules_actor holds neither Dense_1 nor log_stds; every
distribution SACAgent.forward_policy builds has stddev() == clip(fixed_std, std_min, std_max) in every row (recorded per
evaluation as fixed_stddev [evaluation][A], with meta["policy_fixed"]).

The file names do not start with "update_": tests/test_reference_update.py and tests/test_golden_update_gpu.py run every
update_*.npz through the launcher's distribution.  tests/test_policy_fixed_{cpu,gpu}.py read these files.
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
import policy_fixed as PF  # noqa: E402
import policy_modes as PM  # noqa: E402
import variant_recorder as VR  # noqa: E402

ONLY = [a for a in sys.argv[1:] if not a.startswith("-")]


def launcher_config(cfg):
    """the plain oracle Config of the launcher's agent at a FixedConfig's shape and options: what the run is given and the files record"""
    d = {f.name: getattr(cfg, f.name) for f in dataclasses.fields(O.Config)}
    return O.Config(**{**d, "std_parameterization": "exp", "tanh_squash": True})


@contextlib.contextmanager
def reference_fixed(cfg, stddevs):
    """create_states / create_drq with the fixed mode of `cfg`, the run's leaf table for it, and every forward_policy's stddev recorded"""
    over = {"std_parameterization": "fixed", "fixed_std": [float(x) for x in cfg.fixed_std],
            "tanh_squash_distribution": cfg.tanh_squash, "std_min": cfg.std_min, "std_max": cfg.std_max}
    with VR.reference_create_overrides({"policy_kwargs": over}):
        from jax._core import raw
        from serl_launcher.agents.continuous.sac import SACAgent
        fp = SACAgent.__dict__["forward_policy"]

        def forward_policy(self, *a, _orig=fp, **k):
            dist = _orig(self, *a, **k)
            base = dist.distribution if cfg.tanh_squash else dist     # (the tanh distribution's own stddev() is tanh of the Gaussian's)
            stddevs.append(np.asarray(raw(base.stddev()).detach().cpu().numpy(), np.float64))
            return dist
        SACAgent.forward_policy = forward_policy
        paths = RR.theta_flax_paths
        uniform = dataclasses.replace(launcher_config(cfg), std_parameterization="uniform")
        RR.theta_flax_paths = lambda c: {k: v for k, v in paths(uniform).items() if k != PF.LEAF}
        try:
            yield
        finally:
            RR.theta_flax_paths, SACAgent.forward_policy = paths, fp


def main():
    for name in PF.GOLDEN:
        if ONLY and name not in ONLY:
            continue
        os.environ.pop("SERL_JAXSHIM_PRNG", None)
        cfg, B, sched = PF.golden_config(name)
        stddevs = []
        with reference_fixed(cfg, stddevs):
            res = RR.run_reference(launcher_config(cfg), B, sched, GR.PARAM_SEED, GR.BATCH_SEED,
                                   theta_transform=lambda th, c: {k: v for k, v in th.items() if k not in PM.STD_DENSE})
        actor = res["final"]["param_tree"]["modules_actor"]
        assert "Dense_1" not in actor and "log_stds" not in actor and "Dense_0" in actor, sorted(actor)
        with PF.installed():
            assert set(res["final"]["params"]) == set(O.trainable_param_shapes(cfg))
        want = PF.clip_fixed(cfg)
        assert stddevs and all(s.shape == (s.shape[0], cfg.A) for s in stddevs)
        for i, s in enumerate(stddevs):
            assert np.array_equal(s, np.broadcast_to(want, s.shape)), (name, i, s[0], want)
        meta = {"std_parameterization": "fixed", "fixed_std": list(cfg.fixed_std), "tanh_squash_distribution": cfg.tanh_squash,
                "std_min": cfg.std_min, "std_max": cfg.std_max, "backup_entropy": cfg.backup_entropy, "case": PF.GOLDEN[name][0],
                "std_leaves": None, "policy_evaluations": len(stddevs), "rows_per_evaluation": [int(s.shape[0]) for s in stddevs]}
        VR.write(PF.golden_path(name), res, GR.PARAM_SEED, GR.BATCH_SEED, n_sample_key="fixed_n_sample", n_sample=PF.N_SAMPLE,
                 meta_key="policy_fixed", meta=meta, extra={"fixed_stddev": np.stack([s[0] for s in stddevs])})


if __name__ == "__main__":
    main()
