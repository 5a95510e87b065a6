"""Generates the MLP-width fixtures: the REFERENCE's own SACAgent / DrQAgent (serl_launcher/agents/continuous/{sac,drq}.py, built
by its make_sac_agent / make_drq_agent) with critic and policy MLPs of a width other than the launcher's 256, imported
unmodified from its checkout and run under the stand-ins of oracle/jaxshim.  Run in the build container (needs the reference):
    python tests/golden/make_golden_update_widths.py [case ...]

The launcher factories write hidden_dims=[256, 256] into their call of create_states / create_drq (utils/launcher.py:50-116) and
have no width argument, so the two create functions are wrapped AT RUN TIME: the wrapper replaces `hidden_dims` in the
`critic_network_kwargs` / `policy_network_kwargs` the factory passes and calls the reference's function; everything else is what
oracle/ref_update_runner.run_reference does for every other golden (nothing under oracle/ changes).

  widths_update_sac_state_w128.npz  the `sac_state` configuration of make_golden_update.py at hidden = 128; high_utd 2, update, high_utd 1
  widths_update_drq_w320.npz        one camera, 64x64, S = 5, A = 3, hidden = 320; critics, high_utd 2
  widths_init_sac_state_w128.npz    the parameters create_states draws from seed 0 at hidden = 128, state.rng, and one update
                                    from that state (make_golden_init.py's run_agent_case, threefry stream, 512 samples per leaf)

The file names do not start with "update_" / "init_": tests/test_reference_update.py, tests/test_golden_update_gpu.py and
tests/test_init_reference_{cpu,gpu}.py run every update_*.npz / init_*.npz through the launcher factories, which build width 256.
tests/test_mlp_widths_{cpu,gpu}.py read these files.
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import drq_oracle as O  # noqa: E402
from oracle import golden_update as G  # noqa: E402
from oracle import ref_update_runner as RR  # noqa: E402
import variant_recorder as VR  # noqa: E402

PARAM_SEED, BATCH_SEED = 42, 100
# name: (config, batch rows, schedule, sampled elements per large leaf).  make_golden_update.py keeps 2048 samples; the pixel case
# keeps 1024 so that the file stays under 1 MiB.  Every file records its count as "widths_n_sample" (the readers take it from
# the records themselves).
UPDATE_CASES = {
    "sac_state_w128": (O.Config(image_keys=(), S=10, A=4, discount=0.99, warmup=2000, temp_warmup=0, hidden=128), 8,
                       [("high_utd", 2), ("update", ("actor", "critic", "temperature")), ("high_utd", 1)], 2048),
    "drq_w320": (O.Config(image_keys=("image",), H=64, W=64, S=5, A=3, hidden=320), 6, [("critics",), ("high_utd", 2)], 1024),
}
INIT_CASES = {
    "sac_state_w128": (O.Config(image_keys=(), S=10, A=4, discount=0.99, warmup=2000, temp_warmup=0, hidden=128), 8, [("high_utd", 1)]),
}
ONLY = [a for a in sys.argv[1:] if not a.startswith("-")]


def reference_width(h):
    """SACAgent.create_states / DrQAgent.create_drq called with hidden_dims=[h, h] whatever the caller passes"""
    return VR.reference_create_overrides({nk: {"hidden_dims": [h, h]} for nk in ("critic_network_kwargs", "policy_network_kwargs")})


def _check_width(res_tree, cfg):
    """the reference really built width cfg.hidden: its own parameter tree says so"""
    pol = res_tree["modules_actor"]["network"]
    assert tuple(pol["Dense_1"]["kernel"]) == (cfg.hidden, cfg.hidden), pol["Dense_1"]["kernel"]


def main():
    for name, (cfg, B, sched, n_sample) in UPDATE_CASES.items():
        if ONLY and f"update_{name}" not in ONLY:
            continue
        os.environ.pop("SERL_JAXSHIM_PRNG", None)
        with reference_width(cfg.hidden):
            res = RR.run_reference(cfg, B, sched, PARAM_SEED, BATCH_SEED)
        _check_width(res["final"]["param_tree"], cfg)
        VR.write(os.path.join(HERE, f"widths_update_{name}.npz"), res, PARAM_SEED, BATCH_SEED, n_sample_key="widths_n_sample",
                 n_sample=n_sample)
    for name, (cfg, B, sched) in INIT_CASES.items():
        if ONLY and f"init_{name}" not in ONLY:
            continue
        spec = importlib.util.spec_from_file_location("make_golden_init", os.path.join(HERE, "make_golden_init.py"))
        mi = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mi)          # sets SERL_JAXSHIM_PRNG=threefry; records mi.N_SAMPLE = 512 samples, as for init_*.npz
        with reference_width(cfg.hidden):
            rec = mi.run_agent_case(cfg, B, sched)
        assert tuple(rec["init_shape/actor/w2"]) == (cfg.hidden, cfg.hidden), rec["init_shape/actor/w2"]
        rec["widths_n_sample"] = np.int64(mi.N_SAMPLE)
        rec["init_cfg"] = np.frombuffer(repr(G.cfg_to_dict(cfg)).encode(), np.uint8)
        path = os.path.join(HERE, f"widths_init_{name}.npz")
        np.savez_compressed(path, **rec)
        print(name, "->", path, f"{os.path.getsize(path) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
