"""Generates the trained-regime fixtures: the REFERENCE's own SACAgent / DrQAgent update code (serl_launcher/agents/continuous/
{sac,drq}.py, networks/actor_critic_nets.py), imported unmodified from its checkout and run under the stand-ins of oracle/jaxshim in
fp64, on the parameters and batches of tests/trained_regime.py: whole policy columns clipped at std_min and at std_max, saturated
tanh, |Q| of tens, rewards of both signs, stored actions at +-1, and a target copy that differs from the online parameters.  Run in
the build container (needs the reference):
    python tests/golden/make_golden_update_trained.py [name ...]

  trained_update_sac_state_A4.npz   state-only, S = 10, A = 4, 8 rows, lagrange 0.5, mixed masks
  trained_update_drq_64_A5.npz      one camera 64x64, S = 5, A = 5, 6 rows, lagrange 4, masks all one

Both run critics, high_utd 2, update(actor, critic, temperature), critics; the reference's SACAgent has no update_critics (it is
DrQAgent's, drq.py:296-328), so the state-only file records what that method calls, update(networks_to_update={"critic"}), in
its place.  The parameters are trained_regime.trained_like of
O.init_params(param_seed), the target copy is trained_regime.perturb_target of them, the batch of schedule item i is
trained_regime.harden_batch(sample, mode, seed = BATCH_SEED + i); meta["trained"] records the transform's name and seeds, the
lagrange value and the mask mode, and the readers (trained_regime.update_golden) rebuild all three from it.

The file names do not start with "update_": tests/test_reference_update.py and tests/test_golden_update_gpu.py run every
update_*.npz from O.init_params(param_seed) alone.  tests/test_trained_regime_{cpu,gpu}.py read these files.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from oracle import drq_oracle as O  # noqa: E402
from oracle import ref_update_runner as RR  # noqa: E402
import trained_regime as TR  # noqa: E402
import variant_recorder as VR  # noqa: E402

PARAM_SEED, BATCH_SEED = 42, 100
SCHEDULE = [("critics",), ("high_utd", 2), ("update", ("actor", "critic", "temperature")), ("critics",)]
SCHEDULE_STATE = [("update", ("critic",)) if s == ("critics",) else s for s in SCHEDULE]
# name: (config, batch rows, lagrange, mask mode, sampled elements per large leaf).  make_golden_update.py keeps 2048 samples; the
# pixel case keeps fewer so that the file stays under 1 MiB.  Every file records its count as "trained_n_sample".
CASES = {
    "sac_state_A4": (O.Config(image_keys=(), S=10, A=4, discount=0.99, warmup=4, temp_warmup=0), 8, 0.5, "mixed", 1024),
    "drq_64_A5": (O.Config(image_keys=("image",), H=64, W=64, S=5, A=5), 6, 4.0, "one", 512),
}
ONLY = [a for a in sys.argv[1:] if not a.startswith("-")]


def main():
    assert set(CASES) == set(TR.UPDATE_GOLDEN)
    for name, (cfg, B, lam, mode, n_sample) in CASES.items():
        if ONLY and name not in ONLY:
            continue
        os.environ.pop("SERL_JAXSHIM_PRNG", None)
        res = RR.run_reference(cfg, B, SCHEDULE_STATE if cfg.state_only else SCHEDULE, PARAM_SEED, BATCH_SEED,
                               theta_transform=lambda th, c: TR.trained_like(th, c, lam=lam),
                               target_transform=TR.perturb_target, batch_transform=TR.golden_batch_transform(mode))
        meta = {"transform": "trained_like", "seed": TR.TRANSFORM_SEED, "target_transform": "perturb_target",
                "target_seed": TR.TARGET_SEED, "batch_transform": "harden_batch", "batch_seed": TR.BATCH_SEED,
                "lam": lam, "mask_mode": mode}
        VR.write(os.path.join(HERE, f"trained_update_{name}.npz"), res, PARAM_SEED, BATCH_SEED, n_sample_key="trained_n_sample",
                 n_sample=n_sample, meta_key="trained", meta=meta)


if __name__ == "__main__":
    main()
