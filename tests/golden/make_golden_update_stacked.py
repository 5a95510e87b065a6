"""Generates tests/golden/stack2_update_drq_small.npz: the REFERENCE's own DrQAgent (serl_launcher/agents/continuous/drq.py,
built by its make_drq_agent with encoder_type="small") on frame stacks -- obs_horizon T = 2, two cameras, 64x64, S = 5, A = 3,
B = 6 -- imported unmodified from its checkout and run under the stand-ins of oracle/jaxshim with jax.random's own threefry
stream (SERL_JAXSHIM_PRNG=threefry).  Run in the build container (needs the reference):
    python tests/golden/make_golden_update_stacked.py

Recorded, in the form of update_drq_small_encoder.npz (tests/stacked_oracle.py pack / unpack): the parameters the reference's
model_def.init draws from seed 0 for the T = 2 sample observation ("params0": conv_0/kernel (3,3,6,32), the proprio Dense
(10,64)), state.rng before and after, per call the jax.random tape (B*T crop offsets per stream, normals, REDQ indices) and the
info dict, and the final train state.  Schedule: critics, high_utd 2, update{actor,critic,temperature}, critics.

The file name does not start with "update_": tests/test_reference_update.py and tests/test_golden_update_gpu.py run every
tests/golden/update_*.npz through the single-frame batch builder of oracle/golden_update.py.

The SmallEncoder runs with the same call-site adapter as oracle/ref_update_runner.py (EncodingWrapper passes `encode=`, which
SmallEncoder.__call__ does not accept); the networks are built in float32 with the three stand-in replacements of
make_golden_init.py (truncated normal, variance_scaling, the lifted vmap split), the updates run in float64.
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
os.environ["SERL_JAXSHIM_PRNG"] = "threefry"
from oracle import ref_update_runner as RR  # noqa: E402
from oracle import ref_update_shim as R  # noqa: E402
import stacked_oracle as SO  # noqa: E402

T, B, PARAM_SEED, BATCH_SEED = 2, 6, 42, 100
SCHEDULE = [("critics",), ("high_utd", 2), ("update", ("actor", "critic", "temperature")), ("critics",)]


def _make_reference_agent(jnp, cfg):
    import serl_launcher.vision.small_encoders as se
    from serl_launcher.utils.launcher import make_drq_agent
    se_orig = se.SmallEncoder

    class SmallEncoder(se_orig):   # same class name: flax auto-names do not change
        def __call__(self, observations, train=False, encode=True):
            return se_orig.__call__(self, observations, train)

    se.SmallEncoder = SmallEncoder
    try:   # the sample observation ChunkingWrapper(obs_horizon=T) produces: (T, H, W, C) frames, a (T, S) state
        sample_obs = {k: jnp.asarray(np.zeros((T, cfg.H, cfg.W, 3), np.uint8)) for k in cfg.image_keys}
        sample_obs["state"] = jnp.asarray(np.zeros((T, cfg.S // T), np.float32))
        return make_drq_agent(0, sample_obs, jnp.asarray(np.zeros((cfg.A,), np.float32)), image_keys=cfg.image_keys,
                              encoder_type="small", discount=cfg.discount)
    finally:
        se.SmallEncoder = se_orig


def run_reference(cfg):
    import torch
    assert R.reference_available(), "the reference checkout is not present"
    jax = R.install(True)
    spec = importlib.util.spec_from_file_location("make_golden_init", os.path.join(HERE, "make_golden_init.py"))
    mi = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mi)
    mi.patch_standins()
    import jax.numpy as jnp
    from flax.core.frozen_dict import freeze

    jax._core.set_float_dtype(torch.float32)        # the networks are built in float32, as JAX does
    try:
        agent = _make_reference_agent(jnp, cfg)
    finally:
        jax._core.set_float_dtype(torch.float64)
    paths = RR.theta_flax_paths(cfg)
    params0 = {name: np.asarray(RR._get(agent.state.params, p), np.float32) for name, p in paths.items()}
    for k in cfg.image_keys:
        assert params0[f"enc/{k}/conv0/kernel"].shape == (3, 3, 3 * T, 32), params0[f"enc/{k}/conv0/kernel"].shape
    assert params0["enc/proprio/dense/kernel"].shape == (cfg.S, 64)
    rng0 = [int(v) & 0xFFFFFFFF for v in np.asarray(agent.state.rng).reshape(-1)]

    theta = SO.init_params(cfg, T, PARAM_SEED)
    params = jax.tree_map(lambda a: a, agent.state.params)
    for name, path in paths.items():
        cur = RR._get(params, path)
        RR._set(params, path, jnp.asarray(np.asarray(theta[name], np.float64).reshape(tuple(cur.shape))))
    params = jax.tree_map(lambda a: jnp.asarray(np.asarray(a)), params)
    agent = agent.replace(state=agent.state.replace(params=params, target_params=params))

    steps = []
    for i, item in enumerate(SCHEDULE):
        kind = item[0]
        utd = item[1] if kind == "high_utd" else 1
        nets = tuple(item[1]) if kind == "update" else ()
        pb = SO.synth_packed_batch(cfg, T, B, BATCH_SEED + i)
        rb = SO.reference_batch(cfg, T, pb, unpacked=kind == "update", device="cpu")
        conv = lambda d: {k: jnp.asarray(v.numpy()) for k, v in d.items()}   # noqa: E731
        batch = {"observations": conv(rb["observations"]), "next_observations": conv(rb["next_observations"]),
                 "actions": jnp.asarray(pb["action"]), "rewards": jnp.asarray(pb["reward"]), "masks": jnp.asarray(pb["mask"])}
        if kind != "update":
            batch["dones"] = jnp.asarray(1.0 - pb["mask"])
        batch = freeze(batch)
        tape = jax.random.start_tape()
        if kind == "critics":
            agent, info = agent.update_critics(batch)
        elif kind == "high_utd":
            agent, info = agent.update_high_utd(batch, utd_ratio=utd)
        else:
            agent, info = agent.update(batch, networks_to_update=frozenset(nets))
        jax.random.stop_tape()
        noise = SO.parse_noise(cfg, T, B, tape, kind, utd, nets)
        flat = {}
        for k, v in info.items():
            if isinstance(v, dict):
                flat.update({kk: float(np.asarray(vv)) for kk, vv in v.items()})
            else:
                flat[k] = float(np.asarray(v))
        steps.append({"kind": kind, "utd": utd, "nets": nets, "batch": pb, "noise": noise, "info": flat})

    st = agent.state
    final = {"step": int(np.asarray(st.step)), "params": {}, "target": {}, "mu": {}, "nu": {}}
    for name, path in paths.items():
        final["params"][name] = np.asarray(RR._get(st.params, path), np.float64).reshape(-1)
        final["target"][name] = np.asarray(RR._get(st.target_params, path), np.float64).reshape(-1)
    for tx in ("actor", "critic", "temperature"):
        adam = st.opt_states[tx].inner_state[-1][0]
        final["mu"][tx] = {n: np.asarray(RR._get(adam.mu, p), np.float64).reshape(-1) for n, p in paths.items()}
        final["nu"][tx] = {n: np.asarray(RR._get(adam.nu, p), np.float64).reshape(-1) for n, p in paths.items()}
    final["param_tree"] = jax.tree_map(lambda a: tuple(np.shape(a)), st.params)
    final["opt_state_tree"] = jax.tree_map(lambda a: tuple(np.shape(a)), {k: RR._state_dict(v) for k, v in st.opt_states.items()})
    final["rng"] = [int(v) & 0xFFFFFFFF for v in np.asarray(st.rng).reshape(-1)]
    return {"cfg": cfg, "B": B, "schedule": SCHEDULE, "steps": steps, "final": final, "rng0": rng0, "prng": "threefry",
            "params0": params0}


def main():
    cfg = SO.config(("front", "wrist"), 64, 64, 5, 3, T)
    res = run_reference(cfg)
    path = SO.golden_path()
    np.savez_compressed(path, **SO.pack(res, T, PARAM_SEED, BATCH_SEED))
    print(path, f"{os.path.getsize(path) / 1e6:.2f} MB", "final step", res["final"]["step"],
          {k: round(v, 6) for k, v in res["steps"][-1]["info"].items()})


if __name__ == "__main__":
    main()
