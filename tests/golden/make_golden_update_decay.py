"""Generates the weight-decay fixtures of agents with cameras: the REFERENCE's own DrQAgent (serl_launcher/agents/continuous/
{drq,sac}.py, common/optimizers.py:32-46, common/common.py:124-168), imported unmodified from its checkout and run under the
stand-ins of oracle/jaxshim in fp64, with weight_decay in all three optimizers' kwargs (oracle.ref_update_runner.run_reference
passes cfg.opt to create_drq).  Run in the build container (needs the reference):
    python tests/golden/make_golden_update_decay.py [name ...]

optax.adamw decays the whole tree the reference hands it, the pretrained ResNet-10 included: every optimizer step multiplies every
trunk leaf by 1 - sum_t lr_t * wd_t, the target copy follows by the EMA, and forward_target_critic runs the target copy.

  wd_update_drq_one_cam.npz         one camera 64x64, S = 5, A = 3, 6 rows, decay 20 / 30 / 10; critics, high_utd 2, critics
  wd_update_drq_small.npz           the same with the trainable SmallEncoder (no frozen leaf)
  wd_update_sac_pixels_update.npz   the pretrained config through SACAgent.update: all three networks, the critic alone, all three

Every file holds, beside what oracle.golden_update.pack records, the final online and target trunk/conv_init of the run
(`trunk_conv_init`, `trunk_conv_init_target`; absent for the SmallEncoder).  The file names do not start with "update_":
the fixtures of a variant family are kept apart from the update_*.npz sweep.  tests/test_pixel_weight_decay_{cpu,gpu}.py read
these files.
"""
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
import pixel_weight_decay as PW  # noqa: E402
import variant_recorder as VR  # noqa: E402

ONLY = [a for a in sys.argv[1:] if not a.startswith("-")]


def main():
    for name, (cfg, B, sched, n_sample) in PW.GOLDEN.items():
        if ONLY and name not in ONLY:
            continue
        os.environ.pop("SERL_JAXSHIM_PRNG", None)
        res = RR.run_reference(cfg, B, sched, GR.PARAM_SEED, GR.BATCH_SEED)
        extra, meta = {}, {"decay": PW.DECAY}
        if not cfg.small:
            trunk, _ = O.init_params(cfg, GR.PARAM_SEED)
            p0 = trunk["trunk/conv_init"].astype(np.float64).reshape(-1)
            extra = {"trunk_conv_init": res["final"]["trunk_conv_init"], "trunk_conv_init_target": res["final"]["trunk_conv_init_target"]}
            big = np.abs(p0) > 1e-3 * np.abs(p0).max()
            meta["conv_init_ratio"] = float(np.median(extra["trunk_conv_init"][big] / p0[big]))
            meta["conv_init_target_ratio"] = float(np.median(extra["trunk_conv_init_target"][big] / p0[big]))
        VR.write(GR.variant_path("wd", name), res, GR.PARAM_SEED, GR.BATCH_SEED, n_sample_key="wd_n_sample", n_sample=n_sample,
                 meta_key="weight_decay", meta=meta, extra=extra)


if __name__ == "__main__":
    main()
