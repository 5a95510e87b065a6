"""Shared by tests/test_mlp_shapes_cpu.py and tests/test_mlp_shapes_gpu.py: critic and policy MLPs of their own depth and
per-layer widths (serl_agent_create_shapes, hidden_dims of 1 to 4 layers per network).

The fp64 oracle (oracle/drq_oracle.py) states two layers of one width in four functions -- trainable_param_shapes, init_params,
policy_mlp, critic_forward -- and everything else (autograd, apply_gradients, target_update, update_critics, update_high_utd,
agent_helpers.make_pair / leaf_slices) reaches them through the module's globals.  This module holds shape-general versions of the
four, a Config that carries the two width lists, and `installed()`, which puts them on the imported module for the duration of a
test.  At critic_dims == policy_dims == (h, h) the general functions compute what the originals compute, draw for draw and
operation for operation (tests/test_mlp_shapes_cpu.py compares them bit for bit)."""
import contextlib
import dataclasses
import math
import os
import re

import numpy as np
import torch

from oracle import drq_oracle as O
import agent_helpers as AH

GOLDEN_DIR = os.path.join(os.path.dirname(__file__), "golden")
UPDATE_GOLDEN = ("sac_state", "drq")
INIT_GOLDEN = "sac_state"


@dataclasses.dataclass
class ShapeConfig(O.Config):
    critic_dims: tuple = None     # the hidden widths of each MLP, input side first; None: (hidden, hidden)
    policy_dims: tuple = None

    def __post_init__(self):
        super().__post_init__()
        self.critic_dims = tuple(self.critic_dims) if self.critic_dims is not None else (self.hidden, self.hidden)
        self.policy_dims = tuple(self.policy_dims) if self.policy_dims is not None else (self.hidden, self.hidden)


def dims_of(cfg):
    """(critic, policy) widths of any oracle Config"""
    h = cfg.hidden
    return tuple(getattr(cfg, "critic_dims", None) or (h, h)), tuple(getattr(cfg, "policy_dims", None) or (h, h))


_ORIG = {n: getattr(O, n) for n in ("trainable_param_shapes", "init_params", "policy_mlp", "critic_forward")}
_MLP_KERNEL = re.compile(r"(critic|actor)/w\d+")


def trainable_param_shapes(cfg):
    """O.trainable_param_shapes with every MLP layer by layer; order == the arena's."""
    fh, fw = cfg.feat_hw
    E, A, N = cfg.enc_dim, cfg.A, cfg.ensemble
    cd, pd = dims_of(cfg)
    sh = {}
    for k in cfg.image_keys:
        if cfg.small:
            for l in range(4):
                sh[f"enc/{k}/conv{l}/kernel"] = (3, 3, O.SMALL_FEATURES[l], O.SMALL_FEATURES[l + 1])
                sh[f"enc/{k}/conv{l}/bias"] = (O.SMALL_FEATURES[l + 1],)
            sh[f"enc/{k}/dense/kernel"] = (O.SMALL_FEATURES[4], cfg.bottleneck)
        else:
            sh[f"enc/{k}/sle"] = (fh, fw, 512, cfg.sle_features)
            sh[f"enc/{k}/dense/kernel"] = (cfg.sle_dim, cfg.bottleneck)
        sh[f"enc/{k}/dense/bias"] = (cfg.bottleneck,)
        sh[f"enc/{k}/ln/scale"] = (cfg.bottleneck,)
        sh[f"enc/{k}/ln/bias"] = (cfg.bottleneck,)
    fan = E + A
    for j, d in enumerate(cd, 1):
        sh.update({f"critic/w{j}": (N, fan, d), f"critic/b{j}": (N, d), f"critic/ln{j}/scale": (N, d), f"critic/ln{j}/bias": (N, d)})
        fan = d
    if cfg.state_only:
        sh["critic/head/kernel"], sh["critic/head/bias"] = (N, cd[-1], 1), (N,)
    else:
        sh["critic/head/kernel"], sh["critic/head/bias"] = (cd[-1], 1), (1,)
        sh.update({
            "enc/proprio/dense/kernel": (cfg.S, cfg.proprio_dim), "enc/proprio/dense/bias": (cfg.proprio_dim,),
            "enc/proprio/ln/scale": (cfg.proprio_dim,), "enc/proprio/ln/bias": (cfg.proprio_dim,),
        })
    fan = E
    for j, d in enumerate(pd, 1):
        sh.update({f"actor/w{j}": (fan, d), f"actor/b{j}": (d,), f"actor/ln{j}/scale": (d,), f"actor/ln{j}/bias": (d,)})
        fan = d
    sh.update({"actor/mean/kernel": (pd[-1], A), "actor/mean/bias": (A,)})
    if cfg.std_parameterization == "uniform":
        sh["actor/log_stds"] = (A,)
    else:
        sh.update({"actor/logstd/kernel": (pd[-1], A), "actor/logstd/bias": (A,)})
    sh["temp/lagrange"] = ()
    return sh


def init_params(cfg, seed: int = 42, perturb: bool = True):
    """O.init_params over trainable_param_shapes above: the same initialisers in the same draw order."""
    rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed)))

    def normal(shape, std):
        return (rng.standard_normal(shape) * std).astype(np.float32)

    def xavier(shape, fan_in, fan_out):
        a = math.sqrt(6.0 / (fan_in + fan_out))
        return rng.uniform(-a, a, size=shape).astype(np.float32)

    def scale(shape):
        return (1.0 + (0.1 * rng.standard_normal(shape) if perturb else 0.0)).astype(np.float32) * np.ones(shape, np.float32)

    def bias(shape):
        return ((0.1 * rng.standard_normal(shape)) if perturb else np.zeros(shape)).astype(np.float32)

    trunk = {}
    for name, shp in (O.trunk_param_shapes() if cfg.pretrained_trunk else {}).items():
        if len(shp) == 4:
            trunk[name] = normal(shp, math.sqrt(2.0 / (shp[0] * shp[1] * shp[2])))
        elif name.endswith("scale"):
            trunk[name] = scale(shp)
        else:
            trunk[name] = bias(shp)
    theta = {}
    for name, shp in trainable_param_shapes(dataclasses.replace(cfg, std_parameterization="exp")).items():
        if name.endswith("/sle") or ("/conv" in name and name.endswith("kernel")):
            theta[name] = normal(shp, math.sqrt(1.0 / (shp[0] * shp[1] * shp[2])))
        elif name.startswith("enc/") and name.endswith("dense/kernel") and "proprio" not in name:
            theta[name] = normal(shp, math.sqrt(1.0 / shp[0]))
        elif name == "critic/head/kernel" and len(shp) == 3:
            theta[name] = xavier(shp, shp[1], shp[2])
        elif name.endswith("kernel") or (_MLP_KERNEL.fullmatch(name) and name.startswith("actor/")):
            theta[name] = xavier(shp, shp[0], shp[1])
        elif _MLP_KERNEL.fullmatch(name):
            theta[name] = xavier(shp, shp[1], shp[2])
        elif name.endswith("scale"):
            theta[name] = scale(shp)
        elif name == "temp/lagrange":
            theta[name] = np.float32(math.log(math.exp(cfg.temperature_init) - 1.0))
        else:
            theta[name] = bias(shp)
    if cfg.std_parameterization == "uniform":
        theta = {k: theta[k] if k in theta else np.zeros(shp, np.float32) for k, shp in trainable_param_shapes(cfg).items()}
    return trunk, theta


def policy_mlp(th, cfg, enc):
    """MLP (mlp.py:19-31) of the policy: Dense + LayerNorm + activation per entry of hidden_dims -> the last layer's output."""
    h = enc
    for j in range(1, len(dims_of(cfg)[1]) + 1):
        h = O._activate("policy", cfg, O.layer_norm(h @ th[f"actor/w{j}"] + th[f"actor/b{j}"], th[f"actor/ln{j}/scale"], th[f"actor/ln{j}/bias"]))
    return h


def critic_forward(th, cfg, enc, act):
    """Critic with the vmapped ensemble MLP of any depth and the head on its last layer: Q [ensemble, B]."""
    x = torch.cat([enc, act], dim=-1)
    h = torch.einsum("bi,eio->ebo", x, th["critic/w1"]) + th["critic/b1"][:, None, :]
    h = O._activate("critic", cfg, O.layer_norm(h, th["critic/ln1/scale"][:, None, :], th["critic/ln1/bias"][:, None, :]))
    for j in range(2, len(dims_of(cfg)[0]) + 1):
        h = torch.einsum("ebi,eio->ebo", h, th[f"critic/w{j}"]) + th[f"critic/b{j}"][:, None, :]
        h = O._activate("critic", cfg, O.layer_norm(h, th[f"critic/ln{j}/scale"][:, None, :], th[f"critic/ln{j}/bias"][:, None, :]))
    if cfg.state_only:
        return torch.einsum("ebi,eio->ebo", h, th["critic/head/kernel"]).squeeze(-1) + th["critic/head/bias"][:, None]
    return (h @ th["critic/head/kernel"]).squeeze(-1) + th["critic/head/bias"]


GENERAL = {"trainable_param_shapes": trainable_param_shapes, "init_params": init_params, "policy_mlp": policy_mlp,
           "critic_forward": critic_forward}


@contextlib.contextmanager
def installed():
    """the four shape-general functions on the imported oracle module, the originals back on every way out"""
    for n, f in GENERAL.items():
        setattr(O, n, f)
    try:
        yield
    finally:
        for n, f in _ORIG.items():
            setattr(O, n, f)


# ---- the case table: the smallest shapes at which each thing can break -----------------------------------------------------------
# (id, kind, critic widths, policy widths, ensemble, batch rows, UTD > 1 (0: none), critic activation, policy activation)
# kind: "state" (S = 10, A = 4), "frozen1" / "frozen2" (one / two cameras 64x64 on the ResNet-10 trunk, S = 5, A = 3), "small"
CASES = [
    ("c1_state_128_256__64", "state", (128, 256), (64,), 10, 8, 2, "tanh", "tanh"),
    ("c2_state_one_layer_critic", "state", (64,), (192, 64, 320), 3, 65, 5, "relu", "swish"),
    ("c3_frozen_four_layers", "frozen1", (320, 192, 64, 256), (256, 128), 10, 6, 2, "tanh", "tanh"),
    ("c4_small_critic_ne_policy", "small", (256, 256), (128, 128), 2, 6, 2, "tanh", "tanh"),
    ("c5_state_1024_E16_B65", "state", (1024, 64), (64, 1024), 16, 65, 0, "tanh", "tanh"),
    ("c6_frozen2_4x64", "frozen2", (64, 64, 64, 64), (64, 64, 64, 64), 10, 7, 0, "tanh", "tanh"),
]
IDS = [c[0] for c in CASES]
EXTRA_UTD = {"c3_frozen_four_layers": (3,)}     # case 3 runs UTD 2 and 3


def config(kind, critic_dims, policy_dims, ensemble=10, critic_activation="tanh", policy_activation="tanh"):
    kw = dict(critic_dims=tuple(critic_dims), policy_dims=tuple(policy_dims), ensemble=ensemble, critic_activation=critic_activation,
              policy_activation=policy_activation, hidden=critic_dims[0])
    if kind == "state":
        return ShapeConfig(image_keys=(), S=10, A=4, discount=0.99, **kw)
    if kind == "frozen1":
        return ShapeConfig(image_keys=("wrist",), H=64, W=64, S=5, A=3, **kw)
    if kind == "frozen2":
        return ShapeConfig(image_keys=("front", "wrist"), H=64, W=64, S=5, A=3, **kw)
    return ShapeConfig(image_keys=("wrist",), H=64, W=64, S=5, A=3, encoder_type="small", **kw)


def case_config(case):
    """-> (oracle ShapeConfig, batch rows, utd > 1 or 0)"""
    _, kind, cd, pd, ensemble, B, utd, ca, pa = case
    return config(kind, cd, pd, ensemble, ca, pa), B, utd


def make_pair(cfg, B, dtype=torch.float64, seed=42, agent_seed=0, trunk_mode=None, fuse=None):
    """-> (oracle TrainState, AgentCore) holding identical parameters; inside installed()"""
    trunk, theta = init_params(cfg, seed)
    core = AH.make_core(cfg, B, fuse=fuse, trunk_mode=trunk_mode, agent_seed=agent_seed)
    return O.TrainState(cfg, trunk, theta, dtype), AH.load_leaves(core, cfg, trunk, theta)


def mlp_kwargs(dims, **kw):
    """the launcher's critic_network_kwargs / policy_network_kwargs (utils/launcher.py:50-116) with another hidden_dims"""
    return {"activations": "tanh", "use_layer_norm": True, "hidden_dims": list(dims), **kw}


POLICY_KWARGS = {"tanh_squash_distribution": True, "std_parameterization": "exp", "std_min": 1e-5, "std_max": 5}


def sac_agent(critic_dims, policy_dims, seed=0, B=8, S=10, A=4, **kw):
    """make_sac_agent's call of SACAgent.create_states (launcher.py:50-76) with the two hidden_dims and mlp_shapes=True"""
    from serl_amd.agents.sac import SACAgent
    args = dict(policy_kwargs=dict(POLICY_KWARGS), critic_network_kwargs=mlp_kwargs(critic_dims), policy_network_kwargs=mlp_kwargs(policy_dims),
                temperature_init=1e-2, discount=0.99, backup_entropy=False, critic_ensemble_size=10, critic_subsample_size=2,
                batch_size=B, mlp_shapes=True)
    args.update(kw)
    return SACAgent.create_states(seed, np.zeros((S,), np.float32), np.zeros((A,), np.float32), **args)


# ---- tests/golden/shapes_*.npz (tests/golden/make_golden_update_shapes.py) -------------------------------------------------------
def _with_dims(cfg, meta):
    """the launcher's Config a fixture records, with the two lists of its meta block laid over it"""
    d = meta["mlp_shapes"]
    return ShapeConfig(**cfg.__dict__, critic_dims=tuple(d["critic"]), policy_dims=tuple(d["policy"]))


def load_golden(name):
    """-> oracle.golden_update.unpack of shapes_update_<name>.npz, g["cfg"] a ShapeConfig"""
    from oracle import golden_update as G
    g = G.unpack(np.load(os.path.join(GOLDEN_DIR, f"shapes_update_{name}.npz")))
    g["cfg"] = _with_dims(g["cfg"], g["meta"])
    return g


def init_golden():
    """shapes_init_sac_state.npz in the form of init_golden_helpers.load: (npz, cfg, {leaf: (name, record)}, {leaf: shape})"""
    import ast
    import json
    import init_golden_helpers as IG
    from oracle import golden_update as G
    z = np.load(os.path.join(GOLDEN_DIR, f"shapes_init_{INIT_GOLDEN}.npz"))
    assert int(z["shapes_n_sample"]) == IG.N_SAMPLE
    cfg = _with_dims(G.cfg_from_dict(ast.literal_eval(bytes(z["init_cfg"]).decode())), json.loads(str(z["meta"])))
    leaves = {}
    for k in z.files:
        if k.startswith("init/"):
            name, part = k[5:].rsplit("/", 1)
            leaves.setdefault(name, {})[part] = z[k]
    shapes = {k[11:]: tuple(int(s) for s in z[k]) for k in z.files if k.startswith("init_shape/")}
    return z, cfg, {k: (k, v) for k, v in leaves.items()}, shapes


def reference_agent(cfg, B, **kw):
    """golden_replay.reference_agent with the Config's two lists through mlp_shapes=True"""
    import golden_replay as GR
    return GR.reference_agent(cfg, B, critic_network_kwargs=mlp_kwargs(cfg.critic_dims), policy_network_kwargs=mlp_kwargs(cfg.policy_dims),
                              mlp_shapes=True, **kw)
