"""Shared by tests/test_mlp_plain_cpu.py and tests/test_mlp_plain_gpu.py: critic and policy MLPs without LayerNorm
(use_layer_norm=False, mlp.py:29-30; serl_agent_create_layer_norm, mlp_plain=True).

The fp64 oracle (oracle/drq_oracle.py) states LayerNorm in policy_mlp / critic_forward and its leaves in trainable_param_shapes /
init_params; tests/mlp_shapes.py holds shape-general versions of the four.  This module generalises those once more -- a Config
that carries one flag per network, and the four functions reading it -- and `installed()` puts them on the imported oracle module
for the duration of a test.  With both flags True they compute what the mlp_shapes ones compute, draw for draw and operation for
operation (tests/test_mlp_plain_cpu.py compares them bit for bit).

A plain layer is y = act(h @ w + b).  init_params draws as mlp_shapes.init_params does and then leaves out the LayerNorm leaves of
a plain network, so the Dense leaves of a plain agent are those of the LayerNorm agent of the same seed.

ReLU: an fp32 pre-activation must not land on the other side of the kink, so every relu pre-activation of a case has to stay
RELU_MARGIN away from 0 on the fp64 oracle.  The two forward functions report each pre-activation they hand to a relu to the
recorder of `relu_margin()`; check_relu_margin(case) runs a case's oracle calls under it and asserts."""
import contextlib
import dataclasses
import os

import numpy as np
import torch

from oracle import drq_oracle as O
import agent_helpers as AH
import mlp_shapes as MS

GOLDEN_DIR = MS.GOLDEN_DIR
UPDATE_GOLDEN = ("sac_state", "drq")
INIT_GOLDEN = "sac_state"
RELU_MARGIN = 1e-4


@dataclasses.dataclass
class PlainConfig(MS.ShapeConfig):
    critic_layer_norm: bool = True     # use_layer_norm of each network's MLP (mlp.py:29-30)
    policy_layer_norm: bool = True


def layer_norms_of(cfg):
    """(critic, policy) flags of any oracle Config"""
    return bool(getattr(cfg, "critic_layer_norm", True)), bool(getattr(cfg, "policy_layer_norm", True))


_ORIG = {n: getattr(O, n) for n in ("trainable_param_shapes", "init_params", "policy_mlp", "critic_forward")}


def _kept(cfg, name):
    cln, pln = layer_norms_of(cfg)
    return not ((not cln and name.startswith("critic/ln")) or (not pln and name.startswith("actor/ln")))


def trainable_param_shapes(cfg):
    """MS.trainable_param_shapes without the LayerNorm leaves of a plain network; order == the arena's."""
    return {k: v for k, v in MS.trainable_param_shapes(cfg).items() if _kept(cfg, k)}


def init_params(cfg, seed: int = 42, perturb: bool = True):
    """MS.init_params, the LayerNorm leaves of a plain network left out after the draw"""
    trunk, theta = MS.init_params(cfg, seed, perturb)
    return trunk, {k: v for k, v in theta.items() if _kept(cfg, k)}


_RELU = []     # the active recorders of relu_margin()


def _act(which, cfg, pre):
    if _RELU and getattr(cfg, f"{which}_activation") == "relu":
        _RELU[-1].append(float(pre.detach().abs().min()))
    return O._activate(which, cfg, pre)


def policy_mlp(th, cfg, enc):
    """MLP (mlp.py:19-31) of the policy: Dense [+ LayerNorm] + activation per entry of hidden_dims -> the last layer's output."""
    ln = layer_norms_of(cfg)[1]
    h = enc
    for j in range(1, len(MS.dims_of(cfg)[1]) + 1):
        h = h @ th[f"actor/w{j}"] + th[f"actor/b{j}"]
        if ln:
            h = O.layer_norm(h, th[f"actor/ln{j}/scale"], th[f"actor/ln{j}/bias"])
        h = _act("policy", cfg, h)
    return h


def critic_forward(th, cfg, enc, act):
    """Critic with the vmapped ensemble MLP of any depth, with or without LayerNorm, and the head on its last layer: Q [ensemble, B]."""
    ln = layer_norms_of(cfg)[0]
    x = torch.cat([enc, act], dim=-1)
    h = torch.einsum("bi,eio->ebo", x, th["critic/w1"]) + th["critic/b1"][:, None, :]
    if ln:
        h = O.layer_norm(h, th["critic/ln1/scale"][:, None, :], th["critic/ln1/bias"][:, None, :])
    h = _act("critic", cfg, h)
    for j in range(2, len(MS.dims_of(cfg)[0]) + 1):
        h = torch.einsum("ebi,eio->ebo", h, th[f"critic/w{j}"]) + th[f"critic/b{j}"][:, None, :]
        if ln:
            h = O.layer_norm(h, th[f"critic/ln{j}/scale"][:, None, :], th[f"critic/ln{j}/bias"][:, None, :])
        h = _act("critic", cfg, h)
    if cfg.state_only:
        return torch.einsum("ebi,eio->ebo", h, th["critic/head/kernel"]).squeeze(-1) + th["critic/head/bias"][:, None]
    return (h @ th["critic/head/kernel"]).squeeze(-1) + th["critic/head/bias"]


GENERAL = {"trainable_param_shapes": trainable_param_shapes, "init_params": init_params, "policy_mlp": policy_mlp,
           "critic_forward": critic_forward}


@contextlib.contextmanager
def installed():
    """the four general functions on the imported oracle module, the originals back on every way out"""
    for n, f in GENERAL.items():
        setattr(O, n, f)
    try:
        yield
    finally:
        for n, f in _ORIG.items():
            setattr(O, n, f)


@contextlib.contextmanager
def relu_margin():
    """-> a list that receives min |pre-activation| of every relu layer evaluated by the general oracle inside the block"""
    rec = []
    _RELU.append(rec)
    try:
        yield rec
    finally:
        _RELU.pop()


# ---- the case table: the smallest shapes at which the plain rows can go wrong ---------------------------------------------------
# (id, kind, critic widths, policy widths, critic LayerNorm, policy LayerNorm, ensemble, batch rows, UTD > 1 (0: none),
#  critic activation, policy activation, parameter seed)
# kind: "state" (S = 10, A = 4), "frozen1" (one camera 64x64 on the ResNet-10 trunk, S = 5, A = 3), "small" (SmallEncoder).
# Widths: 64 (one column per lane), 256 (blocked), 320 (strided, five columns), 1024.  Rows: 1, 6, 65 (four rows per workgroup:
# 65 leave one in a last workgroup).  Ensembles 2, 10, 16.  A one-layer plain critic has the Q-head dot, the rank-1 backward and
# the loss rider on its only layer.  The relu cases are small on purpose (RELU_MARGIN) and their seeds are chosen for it.
CASES = [
    ("p1_state_both_plain_256", "state", (256, 256), (256, 256), False, False, 10, 8, 2, "tanh", "tanh", 42),
    ("p2_state_one_layer_critic_320_swish", "state", (320,), (64, 128), False, True, 2, 65, 5, "swish", "tanh", 42),
    ("p3_state_four_layer_critic_E16", "state", (64, 320, 256, 64), (64,), False, False, 16, 6, 2, "tanh", "swish", 42),
    ("p4_state_1024_one_row", "state", (1024, 64), (64, 1024), False, False, 2, 1, 0, "swish", "tanh", 42),
    ("p5_state_relu_one_layer", "state", (64,), (64,), False, False, 2, 6, 0, "relu", "relu", 59),
    ("p6_state_policy_plain_relu_beside_ln_critic", "state", (128, 64), (64, 64), True, False, 3, 6, 2, "tanh", "relu", 48),
    ("p7_frozen_critic_plain_beside_ln_policy", "frozen1", (320,), (64, 128), False, True, 10, 6, 2, "swish", "tanh", 42),
    ("p8_small_policy_plain_beside_ln_critic", "small", (256, 256), (128, 64), True, False, 2, 6, 0, "tanh", "tanh", 42),
]
IDS = [c[0] for c in CASES]


def config(kind, critic_dims, policy_dims, critic_layer_norm, policy_layer_norm, ensemble=10, critic_activation="tanh",
           policy_activation="tanh"):
    kw = dict(critic_dims=tuple(critic_dims), policy_dims=tuple(policy_dims), critic_layer_norm=critic_layer_norm,
              policy_layer_norm=policy_layer_norm, ensemble=ensemble, critic_activation=critic_activation,
              policy_activation=policy_activation, hidden=critic_dims[0])
    if kind == "state":
        return PlainConfig(image_keys=(), S=10, A=4, discount=0.99, **kw)
    if kind == "frozen1":
        return PlainConfig(image_keys=("wrist",), H=64, W=64, S=5, A=3, **kw)
    return PlainConfig(image_keys=("wrist",), H=64, W=64, S=5, A=3, encoder_type="small", **kw)


def case_config(case):
    """-> (oracle PlainConfig, batch rows, utd > 1 or 0, parameter seed)"""
    _, kind, cd, pd, cln, pln, ensemble, B, utd, ca, pa, seed = case
    return config(kind, cd, pd, cln, pln, ensemble, ca, pa), B, utd, seed


def make_pair(cfg, B, dtype=torch.float64, seed=42, agent_seed=0, trunk_mode=None, fuse=None):
    """-> (oracle TrainState, AgentCore) holding identical parameters; inside installed()"""
    trunk, theta = init_params(cfg, seed)
    core = AH.make_core(cfg, B, fuse=fuse, trunk_mode=trunk_mode, agent_seed=agent_seed)
    return O.TrainState(cfg, trunk, theta, dtype), AH.load_leaves(core, cfg, trunk, theta)


# ---- the oracle runs of a case, computed once per (case, call, dtype) and shared by the tests that need them ---------------------
# The seeds of the batches and of the noise are those of tests/test_mlp_shapes_gpu.py.
_RUNS = {}


def oracle_run(case, call, dtype=torch.float64):
    """call: "critics", or ("high_utd", utd) -> {"cfg", "B", "seed", "batch", "noise", "state" (the TrainState after the call),
    "info", "aux", "relu" (min |relu pre-activation| per evaluated layer; fp64 runs)}; inside installed().  Unchanged by its readers."""
    key = (case[0], call, dtype)
    if key not in _RUNS:
        cfg, B, _, seed = case_config(case)
        trunk, theta = init_params(cfg, seed)
        st = O.TrainState(cfg, trunk, theta, dtype)
        with relu_margin() as rec:
            if call == "critics":
                b, noise = AH.synth_batch(cfg, B, seed=3), O.make_noise(cfg, B, seed=7)
                info, aux = O.update_critics(st, AH.batch_to_torch(b, dtype), O.noise_to_torch(noise, dtype))
            else:
                utd = call[1]
                b, noise = AH.synth_batch(cfg, B, seed=4), O.make_noise(cfg, B, seed=8, utd_ratio=utd)
                info, aux = O.update_high_utd(st, AH.batch_to_torch(b, dtype), O.noise_to_torch(noise, dtype), utd)
        _RUNS[key] = dict(cfg=cfg, B=B, seed=seed, batch=b, noise=noise, state=st, info=info, aux=aux, relu=list(rec))
    return _RUNS[key]


def calls_of(case):
    """the update calls the GPU parity tests make on a case"""
    return ["critics", ("high_utd", 1)] + ([("high_utd", case[8])] if case[8] > 1 else [])


def check_relu_margin(case):
    """every relu pre-activation of every oracle run of the case is at least RELU_MARGIN from 0 (fp64 oracle alone) -> the worst"""
    worst = float("inf")
    for call in calls_of(case):
        run = oracle_run(case, call)
        has_relu = "relu" in (case[9], case[10])
        assert bool(run["relu"]) == has_relu, (case[0], call)
        for m in run["relu"]:
            assert m >= RELU_MARGIN, f"{case[0]} {call}: a relu pre-activation lies {m:.3g} from 0 (< {RELU_MARGIN:g})"
            worst = min(worst, m)
    return worst


# ---- the reference's call of the create functions ----------------------------------------------------------------------------------
def mlp_kwargs(dims, layer_norm, **kw):
    """the launcher's critic_network_kwargs / policy_network_kwargs (utils/launcher.py:50-116) with another hidden_dims and use_layer_norm"""
    return {"activations": "tanh", "use_layer_norm": bool(layer_norm), "hidden_dims": list(dims), **kw}


def sac_agent(critic_dims, policy_dims, critic_layer_norm, policy_layer_norm, seed=0, B=8, S=10, A=4, **kw):
    """make_sac_agent's call of SACAgent.create_states (launcher.py:50-76) with the two hidden_dims and flags, mlp_shapes and mlp_plain on"""
    from serl_amd.agents.sac import SACAgent
    args = dict(policy_kwargs=dict(MS.POLICY_KWARGS), critic_network_kwargs=mlp_kwargs(critic_dims, critic_layer_norm),
                policy_network_kwargs=mlp_kwargs(policy_dims, policy_layer_norm), temperature_init=1e-2, discount=0.99,
                backup_entropy=False, critic_ensemble_size=10, critic_subsample_size=2, batch_size=B, mlp_shapes=True, mlp_plain=True)
    args.update(kw)
    return SACAgent.create_states(seed, np.zeros((S,), np.float32), np.zeros((A,), np.float32), **args)


# ---- tests/golden/plain_*.npz (tests/golden/make_golden_update_plain.py) ----------------------------------------------------------
def _with_meta(cfg, meta):
    """the launcher's Config a fixture records, with the lists, flags and activations of its meta block laid over it"""
    d = meta["mlp_plain"]
    return PlainConfig(**{**cfg.__dict__, "critic_activation": d["critic_activation"], "policy_activation": d["policy_activation"]},
                       critic_dims=tuple(d["critic"]), policy_dims=tuple(d["policy"]), critic_layer_norm=bool(d["critic_layer_norm"]),
                       policy_layer_norm=bool(d["policy_layer_norm"]))


def meta_of(cfg):
    return {"critic": list(cfg.critic_dims), "policy": list(cfg.policy_dims), "critic_layer_norm": cfg.critic_layer_norm,
            "policy_layer_norm": cfg.policy_layer_norm, "critic_activation": cfg.critic_activation,
            "policy_activation": cfg.policy_activation}


def load_golden(name):
    """-> oracle.golden_update.unpack of plain_update_<name>.npz, g["cfg"] a PlainConfig"""
    from oracle import golden_update as G
    g = G.unpack(np.load(os.path.join(GOLDEN_DIR, f"plain_update_{name}.npz")))
    g["cfg"] = _with_meta(g["cfg"], g["meta"])
    return g


def init_golden():
    """plain_init_sac_state.npz in the form of init_golden_helpers.load: (npz, cfg, {leaf: (name, record)}, {leaf: shape})"""
    import ast
    import json
    import init_golden_helpers as IG
    from oracle import golden_update as G
    z = np.load(os.path.join(GOLDEN_DIR, f"plain_init_{INIT_GOLDEN}.npz"))
    assert int(z["plain_n_sample"]) == IG.N_SAMPLE
    cfg = _with_meta(G.cfg_from_dict(ast.literal_eval(bytes(z["init_cfg"]).decode())), json.loads(str(z["meta"])))
    leaves = {}
    for k in z.files:
        if k.startswith("init/"):
            name, part = k[5:].rsplit("/", 1)
            leaves.setdefault(name, {})[part] = z[k]
    shapes = {k[11:]: tuple(int(s) for s in z[k]) for k in z.files if k.startswith("init_shape/")}
    return z, cfg, {k: (k, v) for k, v in leaves.items()}, shapes


def network_kwargs(cfg):
    """the two network kwargs that make cfg's MLPs, as create_states / create_drq take them"""
    return dict(critic_network_kwargs=mlp_kwargs(cfg.critic_dims, cfg.critic_layer_norm, activations=cfg.critic_activation),
                policy_network_kwargs=mlp_kwargs(cfg.policy_dims, cfg.policy_layer_norm, activations=cfg.policy_activation))


def reference_agent(cfg, B, **kw):
    """golden_replay.reference_agent with the Config's lists and flags through mlp_shapes=True, mlp_plain=True"""
    import golden_replay as GR
    return GR.reference_agent(cfg, B, **network_kwargs(cfg), mlp_shapes=True, mlp_plain=True, **kw)
