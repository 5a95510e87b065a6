"""Generates the LayerNorm-free fixtures: the REFERENCE's own SACAgent / DrQAgent (serl_launcher/agents/continuous/{sac,drq}.py,
built by its make_sac_agent / make_drq_agent) with use_layer_norm=False in the critic's MLP, the policy's, or both
(networks/mlp.py:29-30), imported unmodified from its checkout and run under the stand-ins of oracle/jaxshim.  Run in the build
container (needs the reference):
    python tests/golden/make_golden_update_plain.py [case ...]

The launcher factories write use_layer_norm=True, hidden_dims=[256, 256] and activations=tanh into their call of create_states /
create_drq (utils/launcher.py:50-116), so the two create functions are wrapped AT RUN TIME
(variant_recorder.reference_create_overrides) with each network's own flag, list and activation.  For the duration of a run
RR.theta_flax_paths and the oracle's four shape-bound functions are replaced by the general ones of tests/mlp_plain.py, and
G.cfg_to_dict keeps the record of the Config the launcher's (flags, lists and activations stand in the meta block, under
"mlp_plain").  Every run asserts on the reference's own parameter tree that a plain network holds no LayerNorm_* and the other
network all of them.  Nothing under oracle/ changes.

  plain_update_sac_state.npz  both networks plain, tanh, [256, 256], B = 8; high_utd 2, update (all three), high_utd 1
  plain_update_drq.npz        one camera 64x64 on the frozen trunk, critic plain [320] swish beside a LayerNorm policy [64, 128] tanh,
                              B = 6; critics, high_utd 2
  plain_init_sac_state.npz    seed 0, critic [128, 64] with LayerNorm, policy [64, 64, 128] plain: the initial leaves, state.rng and one
                              high_utd 1 (make_golden_init.py's run_agent_case, threefry stream, 512 samples per leaf)

The names do not start with "update_" / "init_": other tests glob those prefixes.  tests/test_mlp_plain_{cpu,gpu}.py read them.
"""
import contextlib
import dataclasses
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
import mlp_plain as MP  # noqa: E402
import variant_recorder as VR  # noqa: E402

PARAM_SEED, BATCH_SEED = 42, 100
STATE = dict(image_keys=(), S=10, A=4, discount=0.99, warmup=2000, temp_warmup=0)
_OWN = ("critic_dims", "policy_dims", "critic_layer_norm", "policy_layer_norm")
# name: (config, batch rows, schedule, sampled elements per large leaf)
UPDATE_CASES = {
    "sac_state": (MP.PlainConfig(critic_dims=(256, 256), policy_dims=(256, 256), critic_layer_norm=False, policy_layer_norm=False, **STATE),
                  8, [("high_utd", 2), ("update", ("actor", "critic", "temperature")), ("high_utd", 1)], 2048),
    "drq": (MP.PlainConfig(image_keys=("image",), H=64, W=64, S=5, A=3, critic_dims=(320,), policy_dims=(64, 128),
                           critic_layer_norm=False, policy_layer_norm=True, critic_activation="swish"), 6,
            [("critics",), ("high_utd", 2)], 1024),
}
INIT_CASES = {
    "sac_state": (MP.PlainConfig(critic_dims=(128, 64), policy_dims=(64, 64, 128), critic_layer_norm=True, policy_layer_norm=False, **STATE),
                  8, [("high_utd", 1)]),
}
ONLY = [a for a in sys.argv[1:] if not a.startswith("-")]


def theta_flax_paths(cfg):
    """RR.theta_flax_paths with the layer counts and LayerNorm flags of the Config"""
    from serl_amd.agents.flax_tree import theta_paths
    prod = theta_paths(cfg.image_keys, encoder_type=cfg.encoder_type, std_parameterization=cfg.std_parameterization,
                       critic_dims=cfg.critic_dims, policy_dims=cfg.policy_dims, critic_layer_norm=cfg.critic_layer_norm,
                       policy_layer_norm=cfg.policy_layer_norm)
    return {k: prod[RR._product_name(k, cfg.image_keys)][0] for k in MP.trainable_param_shapes(cfg)}


@contextlib.contextmanager
def plain_general(cfg):
    """the reference building cfg's two networks, and the recorder's helpers following it"""
    saved = RR.theta_flax_paths, G.cfg_to_dict
    RR.theta_flax_paths = theta_flax_paths
    G.cfg_to_dict = lambda c: {k: v for k, v in saved[1](c).items() if k not in _OWN}
    over = {f"{net}_network_kwargs": {"hidden_dims": list(dims), "use_layer_norm": bool(ln), "activations": act}
            for net, dims, ln, act in (("critic", cfg.critic_dims, cfg.critic_layer_norm, cfg.critic_activation),
                                       ("policy", cfg.policy_dims, cfg.policy_layer_norm, cfg.policy_activation))}
    try:
        with MP.installed(), VR.reference_create_overrides(over):
            yield
    finally:
        RR.theta_flax_paths, G.cfg_to_dict = saved


def _launcher(cfg):
    """the Config as the record keeps it: the launcher's activations (the real ones stand in the meta block)"""
    return dataclasses.replace(cfg, critic_activation="tanh", policy_activation="tanh")


def _check_tree(tree, cfg):
    """the reference really built the two networks: its own parameter tree says so"""
    for mod, dims, ln in (("modules_critic", cfg.critic_dims, cfg.critic_layer_norm), ("modules_actor", cfg.policy_dims, cfg.policy_layer_norm)):
        net = tree[mod]["network"]
        assert sorted(k for k in net if k.startswith("Dense_")) == [f"Dense_{j}" for j in range(len(dims))], sorted(net)
        assert [tuple(net[f"Dense_{j}"]["kernel"])[-1] for j in range(len(dims))] == list(dims), (mod, net)
        assert sorted(k for k in net if k.startswith("LayerNorm_")) == ([f"LayerNorm_{j}" for j in range(len(dims))] if ln else []), (mod, sorted(net))


def main():
    for name, (cfg, B, sched, n_sample) in UPDATE_CASES.items():
        if ONLY and f"update_{name}" not in ONLY:
            continue
        os.environ.pop("SERL_JAXSHIM_PRNG", None)
        with plain_general(cfg):
            res = RR.run_reference(_launcher(cfg), B, sched, PARAM_SEED, BATCH_SEED)
            _check_tree(res["final"]["param_tree"], cfg)
            VR.write(os.path.join(HERE, f"plain_update_{name}.npz"), res, PARAM_SEED, BATCH_SEED, n_sample_key="plain_n_sample",
                     n_sample=n_sample, meta_key="mlp_plain", meta=MP.meta_of(cfg))
    for name, (cfg, B, sched) in INIT_CASES.items():
        if ONLY and f"init_{name}" not in ONLY:
            continue
        spec = importlib.util.spec_from_file_location("make_golden_init", os.path.join(HERE, "make_golden_init.py"))
        mi = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mi)          # sets SERL_JAXSHIM_PRNG=threefry; records mi.N_SAMPLE = 512 samples, as for init_*.npz
        with plain_general(cfg):
            rec = mi.run_agent_case(_launcher(cfg), B, sched)
            rec["init_cfg"] = np.frombuffer(repr(G.cfg_to_dict(_launcher(cfg))).encode(), np.uint8)
        assert not any(k.startswith("init_shape/actor/ln") for k in rec) and "init_shape/critic/ln2/scale" in rec, sorted(rec)
        m = json.loads(str(rec["meta"]))
        _check_tree(m["param_tree"], cfg)
        m["mlp_plain"] = MP.meta_of(cfg)
        rec["meta"] = np.array(json.dumps(m))
        rec["plain_n_sample"] = np.int64(mi.N_SAMPLE)
        path = os.path.join(HERE, f"plain_init_{name}.npz")
        np.savez_compressed(path, **rec)
        assert os.path.getsize(path) < 1 << 20, path
        print(name, "->", path, f"{os.path.getsize(path) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
