"""Generates tests/golden/bc_*.npz by running the REFERENCE's own behaviour-cloning agent unmodified
(serl_launcher/agents/continuous/bc.py built by make_bc_agent, utils/launcher.py:26-47, encoder_type="resnet-pretrained",
imported from the reference tree) under the third-party stand-ins of oracle/jaxshim, in fp64.  Run in the build container
(needs the reference tree):
    python tests/golden/make_golden_bc.py [case ...]

Per case: the reference agent's trainable leaves are overwritten with oracle.drq_oracle.init_params (the frozen trunk comes
in through the reference's own load_resnet10_params from a synthetic ~/.serl/resnet10_params.pkl; `requests.get` raises, so
nothing is ever downloaded), then `update` runs on reference-format packed batches (oracle.ref_update_runner.synth_packed_batch,
CRC-guarded).  Recorded: the Dropout keep-masks and normals the run drew (from the stand-in's tape; under
SERL_JAXSHIM_PRNG=threefry they are jax.random's own), the info dicts, state.rng, the final trainable params and Adam
moments (golden_update.leaf_record: full or sampled), the parameter / optimizer-state tree, the encoder output of the first
update (for the fp64 NumPy restatement in tests/test_bc_cpu.py), and sample_actions / get_debug_metrics on a fresh batch.

A case may carry the hooks oracle.ref_update_runner.run_reference has: theta_transform(theta, cfg) -> theta on the leaves before
they are patched into the reference agent, and batch_transform(pb, step) -> pb on every synthetic sample (step = the number of
updates for the inference batch).  bc_regime_64 and bc_regime_sat_64 use them to run the reference's BCAgent in the trained regime of
tests/learner_regimes.py (std clipped on both sides in whole columns, saturated tanh, hardened batches).
"""
import json
import os
import pickle
import sys
import tempfile
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import drq_oracle as O  # noqa: E402
from oracle import golden_update as G  # noqa: E402
from oracle import ref_update_runner as RR  # noqa: E402
from oracle import ref_update_shim as R  # noqa: E402

PARAM_SEED, BATCH_SEED, INFER_SEED, SAMPLE_KEY_SEED = 42, 300, 900, 7
# BC's trainable leaves (bc.py: everything behind stop_gradient is frozen) -> flax path in BCAgent.state.params
TRAIN_PATHS = {
    "enc/proprio/dense/kernel": ("modules_actor", "encoder", "Dense_0", "kernel"),
    "enc/proprio/dense/bias": ("modules_actor", "encoder", "Dense_0", "bias"),
    "enc/proprio/ln/scale": ("modules_actor", "encoder", "LayerNorm_0", "scale"),
    "enc/proprio/ln/bias": ("modules_actor", "encoder", "LayerNorm_0", "bias"),
    "actor/w1": ("modules_actor", "network", "Dense_0", "kernel"),
    "actor/b1": ("modules_actor", "network", "Dense_0", "bias"),
    "actor/w2": ("modules_actor", "network", "Dense_1", "kernel"),
    "actor/b2": ("modules_actor", "network", "Dense_1", "bias"),
    "actor/mean/kernel": ("modules_actor", "Dense_0", "kernel"),
    "actor/mean/bias": ("modules_actor", "Dense_0", "bias"),
    "actor/logstd/kernel": ("modules_actor", "Dense_1", "kernel"),
    "actor/logstd/bias": ("modules_actor", "Dense_1", "bias"),
}
CAM_PATHS = {"sle": ("SpatialLearnedEmbeddings_0", "kernel"), "dense/kernel": ("Dense_0", "kernel"),
             "dense/bias": ("Dense_0", "bias"), "ln/scale": ("LayerNorm_0", "scale"), "ln/bias": ("LayerNorm_0", "bias")}
CASES = {
    # two cameras, 2x2 SpatialLearnedEmbeddings: one update, then a 5-step sequence on different batches
    "bc_64": (O.Config(image_keys=("front", "wrist"), H=64, W=64, S=5, A=3), 8, 1),
    "bc_64_seq": (O.Config(image_keys=("front", "wrist"), H=64, W=64, S=5, A=3), 8, 5),
    # one camera
    "bc_one_cam": (O.Config(image_keys=("image",), H=64, W=64, S=7, A=4), 6, 1),
    # 84x84: a 3x3 feature map behind stride-2 convs padded (1, 1) in stages 1 and 2 (tests/shape_edges.py)
    "bc_84": (O.Config(image_keys=("front", "wrist"), H=84, W=84, S=5, A=3), 8, 1),
    # the timed shape: B = 256, two 128x128 cameras, S = 24, A = 6
    "bc_128": (O.Config(image_keys=("front", "wrist"), H=128, W=128, S=24, A=6), 256, 1),
    # the reference's own random stream (jax.random's threefry): masks / eps are drawn from the keys, nothing injected
    "bc_64_threefry": (O.Config(image_keys=("front", "wrist"), H=64, W=64, S=5, A=3), 8, 2),
    # the trained regime (tests/learner_regimes.py: BC_GOLDEN, BC_CFG, BC_B): two updates at A = 5, both clips binding in whole columns
    "bc_regime_64": (O.Config(image_keys=("front", "wrist"), H=64, W=64, S=5, A=5), 8, 2),
    # ... one update with hidden tanh units at exactly +-1 in fp32 as well (BC_GOLDEN_SAT: compared on infos and moments only)
    "bc_regime_sat_64": (O.Config(image_keys=("front", "wrist"), H=64, W=64, S=5, A=5), 8, 1),
}


def hooks(name, cfg):
    """-> (theta_transform, batch_transform, what meta["regime"] says of them) of a case; built only for the case that has them"""
    if not name.startswith("bc_regime_"):
        return None, None, None
    import learner_regimes as LR
    sat_bias = LR.BC_GOLDEN_SAT_BIASES[name]
    assert cfg == LR.BC_CFG
    return (LR.bc_golden_theta_transform(sat_bias), LR.bc_golden_batch_transform(cfg, PARAM_SEED, sat_bias),
            {"transform": "bc_trained_like", "which": "both", "seed": LR.BC_SEED, "sat_bias": list(sat_bias),
             "batch_transform": "harden_bc_batch", "batch_seed": LR.BC_BATCH_SEED})


ONLY = [a for a in sys.argv[1:] if not a.startswith("-")]


def theta_of(cfg, seed):
    """BC's leaves from the DrQ oracle's initialiser (same shapes; the DrQ-only leaves are dropped)."""
    trunk, theta = O.init_params(cfg, seed)
    out = {k: v for k, v in theta.items() if k in TRAIN_PATHS or k.startswith("enc/")}
    return trunk, out


def _get(tree, path):
    for p in path:
        tree = tree[p]
    return tree


def _set(tree, path, value):
    for p in path[:-1]:
        tree = tree[p]
    assert path[-1] in tree, path
    tree[path[-1]] = value


def _make_agent(jax, jnp, cfg, trunk):
    import requests
    from serl_launcher.utils.launcher import make_bc_agent

    def no_network(*a, **k):
        raise RuntimeError("make_golden_bc: the reference tried to download the ResNet-10 weights")

    home = tempfile.mkdtemp(prefix="serl_ref_home_")
    os.makedirs(os.path.join(home, ".serl"))
    with open(os.path.join(home, ".serl", "resnet10_params.pkl"), "wb") as f:
        pickle.dump(RR.pretrained_pickle_tree(trunk), f)
    old_home, old_get = os.environ.get("HOME"), requests.get
    os.environ["HOME"] = home
    requests.get = no_network
    try:
        sample_obs = {k: jnp.asarray(np.zeros((1, cfg.H, cfg.W, 3), np.uint8)) for k in cfg.image_keys}
        sample_obs["state"] = jnp.asarray(np.zeros((1, cfg.S), np.float32))
        return make_bc_agent(0, sample_obs, jnp.asarray(np.zeros((cfg.A,), np.float32)), image_keys=cfg.image_keys,
                             encoder_type="resnet-pretrained")
    finally:
        requests.get = old_get
        if old_home is not None:
            os.environ["HOME"] = old_home


def _shapes(tree):
    if isinstance(tree, dict) or hasattr(tree, "items"):
        return {k: _shapes(v) for k, v in tree.items()}
    if isinstance(tree, (tuple, list)):
        return [_shapes(v) for v in tree]
    if hasattr(tree, "shape"):
        return list(np.shape(tree))
    return type(tree).__name__


def _opt_state_form(jax, s):
    """optax.adam's state: (ScaleByAdamState(count, mu, nu), EmptyState()) -- recorded as names and the count's shape"""
    out = []
    for part in s:
        fields = getattr(part, "_fields", None)
        out.append({"type": type(part).__name__, "fields": list(fields) if fields else []})
    return out


def _masks(tape, cfg, rows, ctx_prefix):
    out = {}
    for k in cfg.image_keys:
        r = tape.take("bernoulli")[0]
        assert r["context"] and r["context"][-1].endswith(f"encoder_{k}/Dropout_0"), r["context"]
        assert r["value"].shape == (rows, cfg.sle_dim) and abs(r["p"] - (1 - cfg.dropout)) < 1e-12
        out[k] = np.asarray(r["value"]).astype(np.uint8)
    return out


def run_case(cfg, B, n_steps, prng, theta_transform=None, batch_transform=None, regime=None):
    jax = R.install(True)
    import jax.numpy as jnp
    from flax.core.frozen_dict import freeze
    import torch

    trunk, theta = theta_of(cfg, PARAM_SEED)
    if theta_transform is not None:
        theta = theta_transform(theta, cfg)
    agent = _make_agent(jax, jnp, cfg, trunk)
    params = jax.tree_map(lambda a: a, agent.state.params)
    first = sorted(cfg.image_keys)[0]
    pe = params["modules_actor"]["encoder"][f"encoder_{first}"]["pretrained_encoder"]
    assert np.array_equal(np.asarray(pe["conv_init"]["kernel"]), trunk["trunk/conv_init"]), "pretrained weights were not patched in"
    for k in cfg.image_keys:
        for leaf, sub in CAM_PATHS.items():
            path = ("modules_actor", "encoder", f"encoder_{k}") + sub
            cur = _get(params, path)
            _set(params, path, jnp.asarray(np.asarray(theta[f"enc/{k}/{leaf}"], np.float64).reshape(tuple(cur.shape))))
    for name, path in TRAIN_PATHS.items():
        cur = _get(params, path)
        _set(params, path, jnp.asarray(np.asarray(theta[name], np.float64).reshape(tuple(cur.shape))))
    params = jax.tree_map(lambda a: jnp.asarray(np.asarray(a)), params)
    agent = agent.replace(state=agent.state.replace(params=params, target_params=params))
    param_paths = sorted("/".join(p) for p in _flat_paths(agent.state.params))
    frozen0 = {"/".join(p): np.asarray(v, np.float64).copy() for p, v in _flat_items(agent.state.params) if p[:3] == ("modules_actor", "encoder", f"encoder_{first}")}
    rng0 = [int(v) & 0xFFFFFFFF for v in np.asarray(agent.state.rng).reshape(-1)]

    rec = {}
    infos = []
    for i in range(n_steps):
        pb = RR.synth_packed_batch(cfg, B, BATCH_SEED + i)
        if batch_transform is not None:
            pb = batch_transform(pb, i)
        batch = RR._to_reference_batch(jnp, freeze, pb, cfg)
        for k, v in pb["frames"].items():
            rec[f"s{i}_crc_{k}"] = np.uint32(zlib.crc32(v.tobytes()))
        tape = jax.random.start_tape()
        agent, info = agent.update(batch)
        jax.random.stop_tape()
        t = RR._Tape(tape)
        masks = _masks(t, cfg, B, "update")
        assert t.done(), [r["kind"] for r in tape[t.i:]]
        for k, m in masks.items():
            rec[f"s{i}_mask_{k}"] = np.packbits(m, axis=None)
        infos.append({k: float(np.asarray(v)) for k, v in info.items()})
        if i == 0:   # the encoder output of this forward pass (fp64 oracle restatement, checked against the loss below)
            th = {kk: torch.tensor(np.asarray(v, np.float64)) for kk, v in theta.items()}
            tp = {kk: torch.tensor(np.asarray(v, np.float64)) for kk, v in trunk.items()}
            feats = {k: O.trunk_forward(tp, torch.tensor(v[:, 0]), torch.float64) for k, v in pb["frames"].items()}
            enc = O.encode(th, cfg, feats, torch.tensor(pb["state"][:, 0], dtype=torch.float64),
                           {k: torch.tensor(m) for k, m in masks.items()}).numpy()
            loss, mse = _np_loss(theta, enc, pb["action"].astype(np.float64))
            assert abs(loss - infos[0]["actor_loss"]) < 1e-9 * max(1.0, abs(loss)), (loss, infos[0])
            assert abs(mse - infos[0]["mse"]) < 1e-9 * max(1.0, abs(mse)), (mse, infos[0])
            if B <= 16:   # (kept small: under ~1 MB per file)
                rec["enc0"] = enc
    for i, inf in enumerate(infos):
        rec[f"s{i}_info"] = np.array([inf["actor_loss"], inf["mse"]], np.float64)

    st = agent.state
    for name, path in TRAIN_PATHS.items():
        for sec, tree in (("params", st.params), ("mu", st.opt_states[0].mu), ("nu", st.opt_states[0].nu)):
            for kind, arr in G.leaf_record(f"{sec}/{name}", np.asarray(_get(tree, path), np.float64)).items():
                rec[f"f_{sec}|{name}|{kind}"] = arr
    # the frozen leaves: unchanged, zero moments (asserted here, where the reference's own state is at hand)
    for p, v in _flat_items(st.params):
        key = "/".join(p)
        if key in frozen0:
            assert np.array_equal(np.asarray(v, np.float64), frozen0[key]), key
    trained = set(TRAIN_PATHS.values())
    for tree in (st.opt_states[0].mu, st.opt_states[0].nu):
        for p, v in _flat_items(tree):
            if p not in trained:
                assert not np.any(np.asarray(v)), p

    # inference on a fresh batch, train=False
    pb = RR.synth_packed_batch(cfg, B, INFER_SEED)
    if batch_transform is not None:
        pb = batch_transform(pb, n_steps)
    for k, v in pb["frames"].items():
        rec[f"inf_crc_{k}"] = np.uint32(zlib.crc32(v.tobytes()))
    obs = {k: jnp.asarray(v[:, :1]) for k, v in pb["frames"].items()}
    obs["state"] = jnp.asarray(pb["state"])
    obs = freeze(obs)
    rec["inf_argmax"] = np.asarray(agent.sample_actions(observations=obs, argmax=True), np.float64)
    key = jax.random.PRNGKey(SAMPLE_KEY_SEED)
    rec["inf_key"] = np.array([int(v) & 0xFFFFFFFF for v in np.asarray(key).reshape(-1)], np.uint32)
    for tag, temp in (("sample", 1.0), ("sample_t025", 0.25)):
        tape = jax.random.start_tape()
        a = agent.sample_actions(observations=obs, seed=key, temperature=temp)
        jax.random.stop_tape()
        (r,) = RR._Tape(tape).take("normal")
        assert r["value"].shape == (B, cfg.A)
        rec[f"inf_{tag}"] = np.asarray(a, np.float64)
        rec[f"inf_{tag}_eps"] = np.asarray(r["value"], np.float64)
    dbg = agent.get_debug_metrics(freeze({"observations": obs, "actions": jnp.asarray(pb["action"])}))
    for k in ("mse", "log_probs", "pi_actions"):
        rec[f"dbg_{k}"] = np.asarray(dbg[k], np.float64)

    meta = {"cfg": G.cfg_to_dict(cfg), "B": B, "steps": n_steps, "param_seed": PARAM_SEED, "batch_seed": BATCH_SEED,
            "infer_seed": INFER_SEED, "prng": prng, "rng0": rng0,
            "rng_final": [int(v) & 0xFFFFFFFF for v in np.asarray(st.rng).reshape(-1)], "final_step": int(np.asarray(st.step)),
            "param_paths": param_paths, "param_tree": _shapes(dict(st.params)),
            "opt_state": _opt_state_form(jax, st.opt_states), "info_keys": sorted(infos[0])}
    if regime is not None:
        meta["regime"] = regime
    rec["meta"] = np.array(json.dumps(meta))
    return rec


def _flat_items(tree, prefix=()):
    if hasattr(tree, "items"):
        for k, v in tree.items():
            yield from _flat_items(v, prefix + (k,))
    else:
        yield prefix, tree


def _flat_paths(tree):
    return [p for p, _ in _flat_items(tree)]


def _np_loss(theta, enc, act):
    """fp64 restatement of bc.py:44-60 (the same as tests/test_bc_cpu.py): no-LayerNorm tanh MLP, diagonal Gaussian"""
    h = np.tanh(enc @ theta["actor/w1"].astype(np.float64) + theta["actor/b1"])
    h = np.tanh(h @ theta["actor/w2"].astype(np.float64) + theta["actor/b2"])
    mean = h @ theta["actor/mean/kernel"].astype(np.float64) + theta["actor/mean/bias"]
    std = np.clip(np.exp(h @ theta["actor/logstd/kernel"].astype(np.float64) + theta["actor/logstd/bias"]), 1e-5, 5.0)
    lp = (-0.5 * ((act - mean) / std) ** 2 - np.log(std) - 0.5 * np.log(2 * np.pi)).sum(-1)
    return float(-lp.mean()), float(((mean - act) ** 2).sum(-1).mean())


def main():
    out_dir = os.path.dirname(os.path.abspath(__file__))
    for name, (cfg, B, n) in CASES.items():
        if ONLY and name not in ONLY:
            continue
        if name.endswith("_threefry"):
            os.environ["SERL_JAXSHIM_PRNG"] = "threefry"
        else:
            os.environ.pop("SERL_JAXSHIM_PRNG", None)
        rec = run_case(cfg, B, n, os.environ.get("SERL_JAXSHIM_PRNG", "philox"), *hooks(name, cfg))
        os.environ.pop("SERL_JAXSHIM_PRNG", None)
        path = os.path.join(out_dir, f"{name}.npz")
        np.savez_compressed(path, **rec)
        print(name, "->", path, f"{os.path.getsize(path) / 1e6:.2f} MB", json.loads(str(rec["meta"]))["final_step"],
              [list(rec[f"s{i}_info"]) for i in range(n)][-1])


if __name__ == "__main__":
    main()
