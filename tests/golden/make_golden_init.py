"""Generates tests/golden/init_*.npz: the parameters the REFERENCE's own create code (DrQAgent.create_drq / SACAgent.create_states
through utils/launcher.py's make_drq_agent / make_sac_agent / make_bc_agent, networks/reward_classifier.py's create_classifier,
imported unmodified from its checkout) initialises from seed 0, `state.rng` after create, and for DrQ / state SAC one update
from that state (nothing injected), recorded as in make_golden_update.py.  Run in the build container (needs the reference):
    python tests/golden/make_golden_init.py

Runs under oracle/jaxshim with SERL_JAXSHIM_PRNG=threefry (jax.random's own key chain).  Three functions of the stand-ins
draw differently from JAX / flax and are replaced IN THIS PROCESS ONLY (oracle/ is unchanged), by NumPy float32 restatements
written here independently of the library:
  * jax.random.truncated_normal: the stand-in draws Philox normals with rejection; JAX draws uniform on
    [erf(lower / sqrt2), erf(upper / sqrt2)) (XLA's float32 erf), then sqrt2 * erf_inv (XLA's ErfInv32) and clips to the
    nextafter of the bounds (jax/_src/random.py _truncated_normal);
  * jax.nn.initializers.variance_scaling: the stand-in computes the scale in float64 and folds it into the uniform's bounds;
    JAX uses float32 ops: var = float32(scale / denominator), uniform(-1, 1) * sqrt(3 * var), truncated_normal * sqrt(var) / 0.8796;
  * flax.linen.vmap(split_rngs={"params": True}): the stand-in folds the member index into a make_rng key; flax splits the
    LazyRng's root key, split(key, N)[i], and keeps the path suffix (flax/core/lift.py vmap), so a member's parameter key is
    _fold_in_static(split(init_rng, N)[i], full module path + counter).
The networks are built with the stand-in's float type set to float32 (as JAX runs them), the updates run in float64.
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
os.environ["SERL_JAXSHIM_PRNG"] = "threefry"
from oracle import drq_oracle as O  # noqa: E402
from oracle import golden_update as G  # noqa: E402
from oracle import ref_update_runner as RR  # noqa: E402
from oracle import ref_update_shim as R  # noqa: E402

SEED, BATCH_SEED = 0, 100
N_SAMPLE = 512     # sampled elements per large leaf (make_golden_update.py keeps 2048): every file stays well under 1 MiB
CASES = {   # name: (config, batch rows, schedule); schedule None = parameters and state.rng only
    "drq_64": (O.Config(image_keys=("front", "wrist"), H=64, W=64, S=5, A=3), 8, [("high_utd", 1)]),
    "drq_small": (O.Config(image_keys=("front", "wrist"), H=64, W=64, S=5, A=3, encoder_type="small"), 8, [("high_utd", 1)]),
    "drq_one_cam": (O.Config(image_keys=("image",), H=64, W=64, S=5, A=3), 8, [("critics",)]),
    "sac_state": (O.Config(image_keys=(), S=10, A=4, discount=0.99, warmup=2000, temp_warmup=0), 8, [("high_utd", 1)]),
    "bc_64": (O.Config(image_keys=("front", "wrist"), H=64, W=64, S=5, A=3), 0, None),
    "classifier": (O.Config(image_keys=("front", "wrist"), H=64, W=64, S=5, A=3), 0, None),
}
ONLY = [a for a in sys.argv[1:] if not a.startswith("-")]

SQRT2 = np.float32(np.sqrt(2.0))


def erf32(x):
    """XLA's float32 erf: clamp to [-4, 4], x * P(x^2) / Q(x^2)"""
    x = np.clip(np.float32(x), np.float32(-4), np.float32(4))
    x2 = np.float32(x * x)
    p = np.float32(-2.72614225801306e-10)
    for c in (2.77068142495902e-08, -2.10102402082508e-06, -5.69250639462346e-05, -7.34990630326855e-04,
              -2.95459980854025e-03, -1.60960333262415e-02):
        p = np.float32(np.float32(p * x2) + np.float32(c))
    q = np.float32(-1.45660718464996e-05)
    for c in (-2.13374055278905e-04, -1.68282697438203e-03, -7.37332916720468e-03, -1.42647390514189e-02):
        q = np.float32(np.float32(q * x2) + np.float32(c))
    return np.float32(np.float32(x * p) / q)


def erfinv32(x):
    """XLA's ErfInv32 (Giles), log1p rounded from float64"""
    x = np.asarray(x, np.float32)
    w = -np.log1p(-(x * x).astype(np.float64)).astype(np.float32)
    lt = w < np.float32(5)
    w = np.where(lt, w - np.float32(2.5), np.sqrt(w) - np.float32(3)).astype(np.float32)
    lo = (2.81022636e-08, 3.43273939e-07, -3.5233877e-06, -4.39150654e-06, 0.00021858087, -0.00125372503, -0.00417768164,
          0.246640727, 1.50140941)
    hi = (-0.000200214257, 0.000100950558, 0.00134934322, -0.00367342844, 0.00573950773, -0.0076224613, 0.00943887047,
          1.00167406, 2.83297682)
    p = np.where(lt, np.float32(lo[0]), np.float32(hi[0])).astype(np.float32)
    for a, b in zip(lo[1:], hi[1:]):
        p = (np.where(lt, np.float32(a), np.float32(b)).astype(np.float32) + (p * w).astype(np.float32)).astype(np.float32)
    return np.where(np.abs(x) == 1, x * np.float32(np.inf), p * x).astype(np.float32)


def uniform32(key, shape, lo, hi):
    from jax import threefry as T
    bits = T.random_bits(key, shape)
    f = ((bits >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1.0)
    lo, hi = np.float32(lo), np.float32(hi)
    return np.maximum(lo, ((f * np.float32(hi - lo)).astype(np.float32) + lo).astype(np.float32)).astype(np.float32)


def truncated_normal32(key, lower, upper, shape):
    lower, upper = np.float32(lower), np.float32(upper)
    a, b = erf32(np.float32(lower / SQRT2)), erf32(np.float32(upper / SQRT2))
    out = (SQRT2 * erfinv32(uniform32(key, shape, a, b))).astype(np.float32)
    return np.clip(out, np.nextafter(lower, np.float32(np.inf)), np.nextafter(upper, np.float32(-np.inf))).astype(np.float32)


_PATCHED = []


def patch_standins():
    if _PATCHED:
        return
    _PATCHED.append(True)
    import jax
    import flax.linen as nn
    from jax import random as jrandom
    from jax._core import asarray, float_dtype
    from jax.nn import initializers as I

    def truncated_normal(key, lower, upper, shape=(), dtype=None):
        return asarray(truncated_normal32(jrandom._tf_key(key), lower, upper, tuple(shape)), dtype or float_dtype())
    jrandom.truncated_normal = truncated_normal

    def variance_scaling(scale, mode, distribution, in_axis=-2, out_axis=-1):
        def init(key, shape, dtype=None):
            shape = tuple(int(s) for s in shape)
            fan_in, fan_out = I._fans(shape, in_axis, out_axis)
            var = np.float32(scale / {"fan_in": fan_in, "fan_out": fan_out, "fan_avg": (fan_in + fan_out) / 2}[mode])
            k = jrandom._tf_key(key)
            if distribution == "truncated_normal":
                v = truncated_normal32(k, -2.0, 2.0, shape) * (np.sqrt(var) / np.float32(0.87962566103423978))
            elif distribution == "uniform":
                v = uniform32(k, shape, -1.0, 1.0) * np.sqrt(np.float32(3) * var)
            else:
                v = uniform32(k, shape, np.nextafter(np.float32(-1), np.float32(0)), 1.0)
                v = (SQRT2 * erfinv32(v)).astype(np.float32) * np.sqrt(var)
            return asarray(np.asarray(v, np.float32), float_dtype())
        return init
    I.variance_scaling = variance_scaling      # lecun_normal() / xavier_uniform() look it up when they are called
    # initialisers the stand-in's layers instantiated when they were defined
    _patch_dataclass_default(nn.Dense, "kernel_init", I.lecun_normal())
    _patch_dataclass_default(nn.Conv, "kernel_init", I.lecun_normal())

    # flax's lifted vmap split: member i gets split(root, N)[i] and keeps the full path as suffix
    Vm, Module = nn._Vmapped, nn.Module
    orig_make_rng = Module.make_rng

    def make_rng(self, name):
        prefix = getattr(self._scope, "path_prefix", None)
        if prefix is None:
            return orig_make_rng(self, name)
        key = (name, self._path)
        c = self._scope.rng_counters.get(key, 0)
        self._scope.rng_counters[key] = c + 1
        from jax import threefry as T
        k = T.flax_fold_in_static(jrandom._tf_key(self._scope.rngs[name]), prefix + tuple(self._path) + (c + 1,))
        return asarray(np.asarray(k, np.int64))
    Module.make_rng = make_rng

    orig_fold_in = jrandom.fold_in

    def vm_call(self, *args, **kwargs):
        sc = self._scope
        root = sc.rngs.get("params")
        members = None if root is None else iter(jrandom.split(root, self.axis_size))
        prefix = tuple(getattr(sc, "path_prefix", ()) or ()) + tuple(self._path)
        orig_scope = nn._Scope

        class MemberScope(orig_scope):
            def __init__(s, params, rngs, initializing):
                super().__init__(params, rngs, initializing)
                s.path_prefix = prefix
        # the stand-in asks for `fold_in(make_rng("params"), i)` (nothing else calls jax.random.fold_in while it initialises
        # the members): answer with the member's split key instead
        jrandom.fold_in = lambda k, i: next(members)
        nn._Scope = MemberScope
        try:
            return Vm._orig_call(self, *args, **kwargs)
        finally:
            jrandom.fold_in, nn._Scope = orig_fold_in, orig_scope
    Vm._orig_call = Vm.__call__
    Vm.__call__ = vm_call
    return jax


def _patch_dataclass_default(cls, field, value):
    import dataclasses
    for c in cls.__mro__:
        fs = getattr(c, "__dataclass_fields__", {})
        if field in fs:
            fs[field].default = value
    params = [f for f in dataclasses.fields(cls)]
    defaults = cls.__init__.__kwdefaults__ or {}
    if field in defaults:
        defaults[field] = value
    names = [p.name for p in params if p.init and not p.kw_only]
    pos = list(cls.__init__.__defaults__ or ())
    if field in names and pos:
        first_default = len(names) - len(pos)
        idx = names.index(field) - first_default
        if 0 <= idx < len(pos):
            pos[idx] = value
            cls.__init__.__defaults__ = tuple(pos)


def product_trunk(cfg):
    from serl_amd.utils.init import init_trunk
    return init_trunk(seed=SEED)


def reference_leaves(tree, paths):
    return {leaf: np.asarray(RR._get(tree, p), np.float32) for leaf, p in paths.items()}


def run_agent_case(cfg, B, sched):
    """make_drq_agent / make_sac_agent(0, ...) as the reference runs them; one update from the state they leave."""
    import torch
    jax = R.install(True)
    patch_standins()
    captured, meta = {}, {}
    trunk = product_trunk(cfg)
    orig_make = RR._make_reference_agent

    def make(jax_, jnp, cfg_, trunk_):
        jax_._core.set_float_dtype(torch.float32)           # the networks are built in float32, as JAX does
        try:
            agent = orig_make(jax_, jnp, cfg_, trunk_)
        finally:
            jax_._core.set_float_dtype(torch.float64)
        captured.update(reference_leaves(agent.state.params, RR.theta_flax_paths(cfg_)))
        meta["rng"] = [int(v) & 0xFFFFFFFF for v in np.asarray(agent.state.rng).reshape(-1)]
        return agent
    RR._make_reference_agent = make
    try:
        res = RR.run_reference(cfg, B, sched, SEED, BATCH_SEED, leaves=(trunk, captured))
    finally:
        RR._make_reference_agent = orig_make
    res["prng"] = "threefry"
    rec = G.pack(res, SEED, BATCH_SEED, n_sample=N_SAMPLE)
    for name, v in captured.items():
        for k, a in G.leaf_record(name, v, N_SAMPLE).items():
            rec[f"init/{name}/{k}"] = a
        rec[f"init_shape/{name}"] = np.asarray(v.shape, np.int64)
    rec["init_rng"] = np.asarray(meta["rng"], np.uint32)
    return rec


def run_bc_case(cfg):
    import importlib.util
    jax = R.install(True)
    patch_standins()
    import torch
    spec = importlib.util.spec_from_file_location("make_golden_bc", os.path.join(os.path.dirname(__file__), "make_golden_bc.py"))
    mb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mb)
    import jax.numpy as jnp
    jax._core.set_float_dtype(torch.float32)
    agent = mb._make_agent(jax, jnp, cfg, product_trunk(cfg))
    jax._core.set_float_dtype(torch.float64)
    from serl_amd.agents.flax_tree import bc_paths
    from serl_amd.utils.init import trunk_shapes
    paths = {k: p for k, p in bc_paths(cfg.image_keys).items() if k not in trunk_shapes()}
    rec = {"init_rng": np.asarray([int(v) & 0xFFFFFFFF for v in np.asarray(agent.state.rng).reshape(-1)], np.uint32)}
    return _init_records(rec, reference_leaves(agent.state.params, paths))


def run_classifier_case(cfg):
    import pickle
    jax = R.install(True)
    patch_standins()
    import torch
    import jax.numpy as jnp
    from serl_launcher.networks.reward_classifier import create_classifier
    from serl_amd.agents.flax_tree import _trunk_paths
    from serl_amd.networks.reward_classifier import _tree_paths
    d = tempfile.mkdtemp()
    pkl = os.path.join(d, "resnet10_params.pkl")
    with open(pkl, "wb") as f:
        pickle.dump(RR.pretrained_pickle_tree(product_trunk(cfg)), f)
    sample = {k: jnp.asarray(np.zeros((1, 1, cfg.H, cfg.W, 3), np.uint8)) for k in cfg.image_keys}
    jax._core.set_float_dtype(torch.float32)
    c = create_classifier(jax.random.PRNGKey(SEED), sample, list(cfg.image_keys), pretrained_encoder_path=pkl)
    jax._core.set_float_dtype(torch.float64)
    keys = tuple(cfg.image_keys)
    paths = {}
    for leaf, p in _tree_paths(keys).items():
        if leaf in _trunk_paths():
            continue
        if leaf.startswith("enc/"):
            _, k, rest = leaf.split("/", 2)
            leaf = f"enc/{keys.index(k)}/{rest}" if k in keys else leaf
        paths[leaf] = p
    return _init_records({}, reference_leaves(c.params.unfreeze(), paths))


def _init_records(rec, leaves):
    for name, v in leaves.items():
        for k, a in G.leaf_record(name, v, N_SAMPLE).items():
            rec[f"init/{name}/{k}"] = a
        rec[f"init_shape/{name}"] = np.asarray(v.shape, np.int64)
    return rec


def main():
    out_dir = os.path.dirname(os.path.abspath(__file__))
    for name, (cfg, B, sched) in CASES.items():
        if ONLY and name not in ONLY:
            continue
        if name.startswith("bc"):
            rec = run_bc_case(cfg)
        elif name == "classifier":
            rec = run_classifier_case(cfg)
        else:
            rec = run_agent_case(cfg, B, sched)
        rec["init_cfg"] = np.frombuffer(repr(G.cfg_to_dict(cfg)).encode(), np.uint8)
        path = os.path.join(out_dir, f"init_{name}.npz")
        np.savez_compressed(path, **rec)
        print(name, "->", path, f"{os.path.getsize(path) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
