"""Shared by tests/test_image_only_cpu.py and tests/test_image_only_gpu.py: agents without the proprio branch
(EncodingWrapper(use_proprio=False), common/encoding.py:53-72; serl_agent_opts.no_proprio, create_drq(image_only=True)).

The fp64 oracle (oracle/drq_oracle.py) states the proprio branch in `encode` and its leaves in trainable_param_shapes / init_params.
This module generalises the three once more, on top of tests/policy_fixed.py (which stacks tests/mlp_plain.py on tests/mlp_shapes.py,
and is what tests/mlp_ragged.py runs): a Config that carries `use_proprio`, whose enc_dim drops proprio_dim when the flag is False, and
`installed()` puts the general functions on the imported oracle module for the duration of a test.  With use_proprio=True they
compute what policy_fixed's compute, draw for draw and operation for operation (tests/test_image_only_cpu.py compares bit for bit).

`encode` is oracle.drq_oracle.encode without the proprio lines: the concatenated camera codes, and `state` is never touched.
init_params draws as policy_fixed.init_params does for the Config (the first kernels at their image-only fan-in) and leaves out
enc/proprio/* after the draw."""
import contextlib
import dataclasses

import numpy as np
import torch

from oracle import drq_oracle as O
import agent_helpers as AH
import policy_fixed as PF


@dataclasses.dataclass
class ImageOnlyConfig(PF.FixedConfig):
    use_proprio: bool = True

    @property
    def enc_dim(self):
        if self.state_only:
            return self.S
        return self.bottleneck * self.n_cam + (self.proprio_dim if self.use_proprio else 0)


def use_proprio_of(cfg):
    return bool(getattr(cfg, "use_proprio", True))


def _kept(cfg, name):
    return use_proprio_of(cfg) or not name.startswith("enc/proprio/")


def trainable_param_shapes(cfg):
    """PF.trainable_param_shapes without enc/proprio/* for an image-only Config (the first kernels follow cfg.enc_dim); order == the arena's"""
    return {k: v for k, v in PF.trainable_param_shapes(cfg).items() if _kept(cfg, k)}


def init_params(cfg, seed: int = 42, perturb: bool = True):
    """PF.init_params, enc/proprio/* left out after the draw"""
    trunk, theta = PF.init_params(cfg, seed, perturb)
    return trunk, {k: v for k, v in theta.items() if _kept(cfg, k)}


_ORIG = {n: getattr(O, n) for n in ("trainable_param_shapes", "init_params", "policy_mlp", "critic_forward", "encode")}


def encode(th, cfg, feats, state, drop_masks=None, stop_gradient=False):
    """EncodingWrapper (encoding.py:26-72) on precomputed trunk features; use_proprio False: cat(codes), `state` unread"""
    if use_proprio_of(cfg) or cfg.state_only:
        return _ORIG["encode"](th, cfg, feats, state, drop_masks, stop_gradient)
    codes = []
    for k in cfg.image_keys:
        if cfg.small:
            f = O.small_encoder_trunk(th, k, feats[k])
        else:
            f = O.sle(feats[k], th[f"enc/{k}/sle"])
            if drop_masks is not None:
                f = torch.where(drop_masks[k].bool(), f / (1.0 - cfg.dropout), torch.zeros_like(f))
        z = f @ th[f"enc/{k}/dense/kernel"] + th[f"enc/{k}/dense/bias"]
        z = torch.tanh(O.layer_norm(z, th[f"enc/{k}/ln/scale"], th[f"enc/{k}/ln/bias"]))
        if stop_gradient:
            z = z.detach()
        codes.append(z)
    return torch.cat(codes, dim=-1)


GENERAL = {**PF.GENERAL, "trainable_param_shapes": trainable_param_shapes, "init_params": init_params, "encode": encode}


@contextlib.contextmanager
def installed():
    """the general functions on the imported oracle module, the originals back on every way out"""
    for n, f in GENERAL.items():
        setattr(O, n, f)
    try:
        yield
    finally:
        for n, f in _ORIG.items():
            setattr(O, n, f)


# ---- the case table (the issue's six): the smallest shapes at which the image-only chain can go wrong ---------------------------------
# frozen trunk or SmallEncoder; one camera (K of the first critic GEMM = 256 + A, no multiple of 64) or two (two camera blocks with
# nothing behind them); 1, 6 and 65 rows (one row; a partial tile; across the 64-row tile and four rows per rider workgroup + 1).
_ADAMW = {k: {"weight_decay": 1e-2, "clip_grad_norm": 0.5} for k in ("actor", "critic", "temperature")}
_D = dict(S=5, ensemble=2, subsample=None, use_proprio=False)
CASES = {
    "c1_frozen_1cam_B6_A3": dict(_D, image_keys=("wrist",), H=32, W=32, A=3, rows=6),
    "c2_frozen_2cam_33x47_B65_A5_E10": dict(_D, image_keys=("wrist", "front"), H=33, W=47, A=5, rows=65, ensemble=10, subsample=2),
    "c3_small_1cam_B6_A3_adamw_clip": dict(_D, image_keys=("wrist",), H=32, W=32, A=3, rows=6, encoder_type="small", opt=_ADAMW),
    "c4_small_stack2_2cam_47x33_B65_A4": dict(_D, image_keys=("wrist", "front"), H=47, W=33, A=4, rows=65, encoder_type="small", num_stack=2),
    "c5_frozen_1cam_B1_A1": dict(_D, image_keys=("wrist",), H=32, W=32, A=1, rows=1),
    "c6_frozen_plain_swish_critic_320_ragged_policy_uniform": dict(
        _D, image_keys=("wrist",), H=32, W=32, A=3, rows=6, critic_dims=(320,), policy_dims=(65, 127), critic_layer_norm=False,
        critic_activation="swish", std_parameterization="uniform"),
}
IDS = [k for k in CASES if "stack2" not in k]      # (the frame-stack case runs through tests/stacked_oracle.py: see test_image_only_gpu.py)
PARAM_SEED = 42


def case_config(name, **over):
    """-> (ImageOnlyConfig, batch rows)"""
    c = dict(CASES[name], **over)
    rows = c.pop("rows")
    c.pop("num_stack", None)
    if "critic_dims" in c:
        c.setdefault("hidden", c["critic_dims"][0])
    return ImageOnlyConfig(**c), rows


def make_core(cfg, B, *, fuse=None, trunk_mode=None, agent_seed=0, num_stack=1):
    """agent_helpers.make_core with serl_agent_opts.no_proprio (and ragged_widths where a width is off the grid) set"""
    from serl_amd.agents.core import AgentCore
    fixed = getattr(cfg, "fixed_std", None)
    dims = [d for net in (getattr(cfg, "critic_dims", None) or (cfg.hidden,), getattr(cfg, "policy_dims", None) or (cfg.hidden,)) for d in net]
    with AH.chain_fuse(fuse):
        core = AgentCore(encoder_type=cfg.encoder_type, n_cam=cfg.n_cam, H=cfg.H, W=cfg.W, state_dim=cfg.S * num_stack, act_dim=cfg.A, batch=B,
                         ensemble=cfg.ensemble, hidden=cfg.hidden, discount=cfg.discount, tau=cfg.tau, lr=cfg.lr,
                         warmup_steps=cfg.warmup, dropout=cfg.dropout, std_min=cfg.std_min, std_max=cfg.std_max,
                         target_entropy=cfg.target_entropy, seed=agent_seed,
                         temp_warmup_steps=-1 if cfg.temp_warmup is None else cfg.temp_warmup,
                         critic_subsample_size=cfg.subsample, backup_entropy=cfg.backup_entropy, optimizers=cfg.opt,
                         std_parameterization=cfg.std_parameterization if fixed is None else "fixed",
                         fixed_std=None if fixed is None else np.asarray(fixed, np.float32), tanh_squash_distribution=cfg.tanh_squash,
                         critic_activation=cfg.critic_activation, policy_activation=cfg.policy_activation,
                         critic_dims=getattr(cfg, "critic_dims", None), policy_dims=getattr(cfg, "policy_dims", None),
                         critic_layer_norm=getattr(cfg, "critic_layer_norm", True), policy_layer_norm=getattr(cfg, "policy_layer_norm", True),
                         ragged=any(d % 64 for d in dims), use_proprio=use_proprio_of(cfg), num_stack=num_stack)
    if trunk_mode is not None:
        core.set_trunk_mode(trunk_mode)
    return core


def make_pair(cfg, B, dtype=torch.float64, seed=PARAM_SEED, fuse=None):
    """-> (oracle TrainState, AgentCore) holding identical leaves; inside installed()"""
    trunk, theta = init_params(cfg, seed)
    return O.TrainState(cfg, trunk, theta, dtype), AH.load_leaves(make_core(cfg, B, fuse=fuse), cfg, trunk, theta)


_RUNS = {}


def oracle_run(name, call, dtype=torch.float64):
    """call: "critics" or ("high_utd", utd) -> {"cfg", "B", "seed", "batch", "noise", "state" (the TrainState after the call), "info",
    "aux"}; computed once per (case, call, dtype), inside installed(), unchanged by its readers.  Batch and noise seeds:
    tests/mlp_plain.py's."""
    key = (name, call, dtype)
    if key not in _RUNS:
        cfg, B = case_config(name)
        trunk, theta = init_params(cfg, PARAM_SEED)
        st = O.TrainState(cfg, trunk, theta, dtype)
        if call == "critics":
            b, noise = AH.synth_batch(cfg, B, seed=3), O.make_noise(cfg, B, seed=7)
            info, aux = O.update_critics(st, AH.batch_to_torch(b, dtype), O.noise_to_torch(noise, dtype))
        else:
            utd = call[1]
            b, noise = AH.synth_batch(cfg, B, seed=4), O.make_noise(cfg, B, seed=8, utd_ratio=utd)
            info, aux = O.update_high_utd(st, AH.batch_to_torch(b, dtype), O.noise_to_torch(noise, dtype), utd)
        _RUNS[key] = dict(cfg=cfg, B=B, seed=PARAM_SEED, batch=b, noise=noise, state=st, info=info, aux=aux)
    return _RUNS[key]


# ---- case 4, the frame stack: the oracle's agent widened as tests/stacked_oracle.py does ----------------------------------------------
# _compare_state (tests/test_agent_gpu.py) holds the 99.9th percentile of a leaf's error to TOL, which in a leaf of fewer than 1000
# elements is its worst element; Adam's first step -lr g / (|g| + 1e-8) is ill-conditioned in an element whose gradient is of the
# size of its epsilon (that helper's docstring).  So the batch seed of case 4 is chosen on the CPU such that on the fp64 oracle every
# non-zero gradient element of such a leaf at the first step is at least ADAM_MARGIN = 100 epsilon in size
# (tests/test_image_only_cpu.py asserts it; seed 30 has an element of 1.1e-8 in enc/front/conv1/bias).
ADAM_MARGIN = 1e-6
STACK_SEED = 35


def stack_pair(fuse=None, use_proprio=False, core=True):
    """case 4 as an (oracle TrainState, AgentCore with num_stack 2) pair -> (cfg, the Config of the batch's widths, T, B, st, core);
    core False: no agent is made (CPU)"""
    import stacked_oracle as SO
    name, T = "c4_small_stack2_2cam_47x33_B65_A4", 2
    cfg, B = case_config(name, use_proprio=use_proprio)
    wcfg = O.Config(image_keys=cfg.image_keys, H=cfg.H, W=cfg.W, S=cfg.S * T, A=cfg.A, encoder_type="small")   # S: the flattened width
    if use_proprio:
        cfg = ImageOnlyConfig(**{**cfg.__dict__, "S": cfg.S * T})
    _, theta = init_params(cfg, PARAM_SEED)
    wide = SO.init_params(wcfg, T, PARAM_SEED)
    for k in cfg.image_keys:
        theta[f"enc/{k}/conv0/kernel"] = wide[f"enc/{k}/conv0/kernel"]
    st = O.TrainState(cfg, {}, theta, torch.float64)
    if not core:
        return cfg, wcfg, T, B, st, None
    c = make_core(ImageOnlyConfig(**{**cfg.__dict__, "S": wcfg.S // T}), B, fuse=fuse, num_stack=T)
    SO.load_theta(c, cfg, theta)
    return cfg, wcfg, T, B, st, c


def stack_batch(cfg, wcfg, T, B, utd, seed=None):
    """-> (packed batch, noise, cropped frames) of case 4's calls"""
    import stacked_oracle as SO
    seed = STACK_SEED if seed is None else seed
    pb = SO.synth_packed_batch(wcfg, T, B, seed)
    noise = SO.make_noise(cfg, T, B, seed=seed + 10, utd_ratio=utd)
    return pb, noise, SO.cropped(wcfg, T, pb, noise["crop_obs"], noise["crop_next"])


def stack_first_step_margin(seed=None):
    """the smallest non-zero |gradient element| over the leaves of fewer than 1000 elements at case 4's update_critics (fp64)"""
    import stacked_oracle as SO
    cfg, wcfg, T, B, st, _ = stack_pair(core=False)
    pb, noise, fr = stack_batch(cfg, wcfg, T, B, 1, seed)
    _, aux = O.update_critics(st, SO.oracle_batch(wcfg, T, pb, fr), O.noise_to_torch(noise, torch.float64))
    return min(float(g.abs()[g != 0].min()) for g in aux["grads"].values() if g.numel() < 1000 and bool((g != 0).any()))


SECTIONS = ("params", "target_params", "opt/critic/mu", "opt/critic/nu", "opt/actor/mu", "opt/actor/nu", "opt/temperature/mu",
            "opt/temperature/nu")


def all_bits(core):
    return {(sec, leaf): core.get(sec, leaf).copy() for leaf in core.leaves for sec in SECTIONS}


# ---- the reference's call of create_drq ----------------------------------------------------------------------------------------------
def drq_agent(image_keys=("wrist",), H=32, W=32, S=5, A=3, B=6, seed=0, encoder_type="resnet-pretrained", **kw):
    """make_drq_agent's call of DrQAgent.create_drq (utils/launcher.py:79-116) with image_only=True, use_proprio=False unless said"""
    from serl_amd.agents.drq import DrQAgent
    obs = {k: np.zeros((H, W, 3), np.uint8) for k in image_keys}
    obs["state"] = np.zeros((S,), np.float32)
    args = dict(encoder_type=encoder_type, use_proprio=False, image_only=True, image_keys=tuple(image_keys), batch_size=B,
                critic_network_kwargs={"activations": "tanh", "use_layer_norm": True, "hidden_dims": [256, 256]},
                policy_network_kwargs={"activations": "tanh", "use_layer_norm": True, "hidden_dims": [256, 256]},
                policy_kwargs={"tanh_squash_distribution": True, "std_parameterization": "exp", "std_min": 1e-5, "std_max": 5},
                temperature_init=1e-2, discount=0.96, backup_entropy=False, critic_ensemble_size=10, critic_subsample_size=2)
    args.update(kw)
    return DrQAgent.create_drq(seed, obs, np.zeros((A,), np.float32), **args)


def flat_batch(image_keys, H, W, S, A, B, seed, state=None):
    """a replay-format batch of unpacked frames as device tensors (what the update calls take); `state`: a value every state element takes (None: normal draws)"""
    rng = np.random.default_rng(seed)
    t = lambda a: torch.tensor(a, device="cuda")   # noqa: E731
    st = lambda: t(rng.standard_normal((B, S)).astype(np.float32) if state is None else np.full((B, S), state, np.float32))   # noqa: E731
    return {"observations": {**{k: t(rng.integers(0, 256, (B, 1, H, W, 3), dtype=np.uint8)) for k in image_keys}, "state": st()},
            "next_observations": {**{k: t(rng.integers(0, 256, (B, 1, H, W, 3), dtype=np.uint8)) for k in image_keys}, "state": st()},
            "actions": t(rng.uniform(-0.9, 0.9, (B, A)).astype(np.float32)), "rewards": t((rng.random(B) < 0.3).astype(np.float32)),
            "masks": t((rng.random(B) < 0.9).astype(np.float32))}


# ---- tests/golden/imgonly_*.npz (tests/golden/make_golden_update_image_only.py): the reference's own create_drq(use_proprio=False) --------
GOLDEN_DIR = PF.GOLDEN_DIR
UPDATE_GOLDEN = ("drq", "drq_small")


def _with_meta(cfg, meta):
    """the launcher's Config a fixture records, with the flag of its meta block laid over it"""
    return ImageOnlyConfig(**cfg.__dict__, use_proprio=bool(meta["image_only"]["use_proprio"]))


def load_golden(name):
    """-> oracle.golden_update.unpack of imgonly_update_<name>.npz, g["cfg"] an ImageOnlyConfig"""
    import os
    from oracle import golden_update as G
    g = G.unpack(np.load(os.path.join(GOLDEN_DIR, f"imgonly_update_{name}.npz")))
    g["cfg"] = _with_meta(g["cfg"], g["meta"])
    return g


def init_golden():
    """imgonly_init_drq.npz in the form of init_golden_helpers.load: (npz, cfg, {leaf: (name, record)}, {leaf: shape})"""
    import ast
    import json
    import os
    import init_golden_helpers as IG
    from oracle import golden_update as G
    z = np.load(os.path.join(GOLDEN_DIR, "imgonly_init_drq.npz"))
    assert int(z["imgonly_n_sample"]) == IG.N_SAMPLE
    cfg = _with_meta(G.cfg_from_dict(ast.literal_eval(bytes(z["init_cfg"]).decode())), json.loads(str(z["meta"])))
    leaves = {}
    for k in z.files:
        if k.startswith("init/"):
            name, part = k[5:].rsplit("/", 1)
            leaves.setdefault(name, {})[part] = z[k]
    shapes = {IG.product_name(k[11:], cfg.image_keys): tuple(int(s) for s in z[k]) for k in z.files if k.startswith("init_shape/")}
    return z, cfg, {IG.product_name(k, cfg.image_keys): (k, v) for k, v in leaves.items()}, shapes


def reference_agent(cfg, B, **kw):
    """golden_replay.reference_agent with the Config's flag through image_only=True"""
    import golden_replay as GR
    return GR.reference_agent(cfg, B, use_proprio=bool(cfg.use_proprio), image_only=True, **kw)
