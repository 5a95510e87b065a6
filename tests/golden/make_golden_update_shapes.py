"""Generates the MLP-shape fixtures: the REFERENCE's own SACAgent / DrQAgent (serl_launcher/agents/continuous/{sac,drq}.py, built
by its make_sac_agent / make_drq_agent) with critic and policy MLPs of their own depth and per-layer widths, imported unmodified
from its checkout and run under the stand-ins of oracle/jaxshim.  Run in the build container (needs the reference):
    python tests/golden/make_golden_update_shapes.py [case ...]

The launcher factories write hidden_dims=[256, 256] into their call of create_states / create_drq (utils/launcher.py:50-116), so
the two create functions are wrapped AT RUN TIME (variant_recorder.reference_create_overrides) with each network's own list.
oracle.ref_update_runner.run_reference maps leaves to flax paths and sizes them through oracle.drq_oracle, both of which state two
layers: for the duration of a run RR.theta_flax_paths and the oracle's four shape-bound functions are replaced by the
shape-general ones of tests/mlp_shapes.py, and G.cfg_to_dict keeps the record of the Config the launcher's (the two lists stand
in the meta block, under "mlp_shapes").  Nothing under oracle/ changes.

  shapes_update_sac_state.npz  critic [128, 256, 64], policy [192], B = 8; high_utd 2, update (all three), high_utd 1
  shapes_update_drq.npz        one camera 64x64, critic [320], policy [64, 128, 64], B = 6; critics, high_utd 2
  shapes_init_sac_state.npz    seed 0, critic [128, 64], policy [64, 64, 128]: the initial leaves, state.rng and one high_utd 1
                               (make_golden_init.py's run_agent_case, threefry stream, 512 samples per leaf)

The names do not start with "update_" / "init_": other tests glob those prefixes.  tests/test_mlp_shapes_{cpu,gpu}.py read them.
"""
import contextlib
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import golden_update as G  # noqa: E402
from oracle import ref_update_runner as RR  # noqa: E402
import mlp_shapes as MS  # noqa: E402
import variant_recorder as VR  # noqa: E402

PARAM_SEED, BATCH_SEED = 42, 100
STATE = dict(image_keys=(), S=10, A=4, discount=0.99, warmup=2000, temp_warmup=0)
# name: (config, batch rows, schedule, sampled elements per large leaf)
UPDATE_CASES = {
    "sac_state": (MS.ShapeConfig(critic_dims=(128, 256, 64), policy_dims=(192,), **STATE), 8,
                  [("high_utd", 2), ("update", ("actor", "critic", "temperature")), ("high_utd", 1)], 2048),
    "drq": (MS.ShapeConfig(image_keys=("image",), H=64, W=64, S=5, A=3, critic_dims=(320,), policy_dims=(64, 128, 64)), 6,
            [("critics",), ("high_utd", 2)], 1024),
}
INIT_CASES = {
    "sac_state": (MS.ShapeConfig(critic_dims=(128, 64), policy_dims=(64, 64, 128), **STATE), 8, [("high_utd", 1)]),
}
ONLY = [a for a in sys.argv[1:] if not a.startswith("-")]


def theta_flax_paths(cfg):
    """RR.theta_flax_paths with the layer counts of the Config"""
    from serl_amd.agents.flax_tree import theta_paths
    prod = theta_paths(cfg.image_keys, encoder_type=cfg.encoder_type, std_parameterization=cfg.std_parameterization,
                       critic_dims=cfg.critic_dims, policy_dims=cfg.policy_dims)
    return {k: prod[RR._product_name(k, cfg.image_keys)][0] for k in MS.trainable_param_shapes(cfg)}


@contextlib.contextmanager
def shape_general(cfg):
    """the reference building cfg's two lists, and the recorder's helpers following it"""
    saved = RR.theta_flax_paths, G.cfg_to_dict
    RR.theta_flax_paths = theta_flax_paths
    G.cfg_to_dict = lambda c: {k: v for k, v in saved[1](c).items() if k not in ("critic_dims", "policy_dims")}
    try:
        with MS.installed(), VR.reference_create_overrides({"critic_network_kwargs": {"hidden_dims": list(cfg.critic_dims)},
                                                            "policy_network_kwargs": {"hidden_dims": list(cfg.policy_dims)}}):
            yield
    finally:
        RR.theta_flax_paths, G.cfg_to_dict = saved


def _meta(cfg):
    return {"critic": list(cfg.critic_dims), "policy": list(cfg.policy_dims)}


def _check_shapes(tree, cfg):
    """the reference really built the two lists: its own parameter tree says so"""
    for mod, dims in (("modules_critic", cfg.critic_dims), ("modules_actor", cfg.policy_dims)):
        net = tree[mod]["network"]
        assert sorted(k for k in net if k.startswith("Dense_")) == [f"Dense_{j}" for j in range(len(dims))], sorted(net)
        assert [tuple(net[f"Dense_{j}"]["kernel"])[-1] for j in range(len(dims))] == list(dims), (mod, net)


def main():
    for name, (cfg, B, sched, n_sample) in UPDATE_CASES.items():
        if ONLY and f"update_{name}" not in ONLY:
            continue
        os.environ.pop("SERL_JAXSHIM_PRNG", None)
        with shape_general(cfg):
            res = RR.run_reference(cfg, B, sched, PARAM_SEED, BATCH_SEED)
            _check_shapes(res["final"]["param_tree"], cfg)
            VR.write(os.path.join(HERE, f"shapes_update_{name}.npz"), res, PARAM_SEED, BATCH_SEED, n_sample_key="shapes_n_sample",
                     n_sample=n_sample, meta_key="mlp_shapes", meta=_meta(cfg))
    for name, (cfg, B, sched) in INIT_CASES.items():
        if ONLY and f"init_{name}" not in ONLY:
            continue
        spec = importlib.util.spec_from_file_location("make_golden_init", os.path.join(HERE, "make_golden_init.py"))
        mi = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mi)          # sets SERL_JAXSHIM_PRNG=threefry; records mi.N_SAMPLE = 512 samples, as for init_*.npz
        with shape_general(cfg):
            rec = mi.run_agent_case(cfg, B, sched)
            rec["init_cfg"] = np.frombuffer(repr(G.cfg_to_dict(cfg)).encode(), np.uint8)
        assert tuple(rec["init_shape/actor/w3"]) == cfg.policy_dims[1:], rec["init_shape/actor/w3"]
        m = json.loads(str(rec["meta"]))
        _check_shapes(m["param_tree"], cfg)
        m["mlp_shapes"] = _meta(cfg)
        rec["meta"] = np.array(json.dumps(m))
        rec["shapes_n_sample"] = np.int64(mi.N_SAMPLE)
        path = os.path.join(HERE, f"shapes_init_{name}.npz")
        np.savez_compressed(path, **rec)
        assert os.path.getsize(path) < 1 << 20, path
        print(name, "->", path, f"{os.path.getsize(path) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
