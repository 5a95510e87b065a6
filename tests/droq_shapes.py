"""Shared by tests/test_droq_shapes_{cpu,gpu}.py: MLP Dropout at every served shape (mlp_dropout="any", serl_agent_opts.dropout_any)
-- the DROP rows of the plain, ragged and four-wave families (serl_amd/csrc/heads.hip, ln_wide.h) and masks laid out by true widths.

The oracle is the shape-general fp64 one of tests/image_only.py (any depth and width, LayerNorm flags, use_proprio) with this
file's own Dropout hook: policy_mlp / critic_forward below are tests/mlp_plain.py's with one mask popped per (site, layer), applied as
x * m / keep in front of the LayerNorm where the layer has one and in front of the activation where it has none (mlp.py:27-31).
A call's masks are {site: [u8[rows, d_l] per layer]} over the sites that draw, in the reference's draw order (mlp_dropout.site_order)."""
import contextlib
import functools

import numpy as np
import torch

from oracle import drq_oracle as O
from serl_amd._lib_agent import MLP_SITE_NETWORK
import agent_helpers as AH
import image_only as IO
import mlp_activations as MA
import mlp_dropout as MD
import mlp_plain as MP
import mlp_shapes as MS

_S = dict(image_keys=(), discount=0.99, S=10, A=4, ensemble=2)
# name -> ImageOnlyConfig kwargs, rows, (critic rate, policy rate); "kink": start from mlp_activations.kink_margin's leaves
CASES = {
    "shapes": dict(_S, critic_dims=(128, 64, 192), policy_dims=(64,), rows=6, rates=(0.1, 0.2)),
    "ragged": dict(_S, critic_dims=(65, 127), policy_dims=(65, 127), rows=65, rates=(0.1, 0.1)),
    "plain_swish_critic": dict(_S, critic_dims=(320,), policy_dims=(64, 64), critic_layer_norm=False, critic_activation="swish", rows=65,
                               rates=(0.1, 0.1)),
    # (relu on the LayerNorm side of the pairing: a dropped element of a plain relu layer IS the kink, pre-activation exactly 0)
    "plain_policy_relu_critic": dict(_S, critic_dims=(64, 64), policy_dims=(320,), policy_layer_norm=False, critic_activation="relu", rows=65,
                                     rates=(0.1, 0.1), kink=True),
    "wide": dict(_S, critic_dims=(1088, 64), policy_dims=(64, 1088), rows=65, rates=(0.1, 0.1)),
    "wide_one_row": dict(_S, critic_dims=(1088, 64), policy_dims=(64, 1088), rows=1, rates=(0.1, 0.1)),
    "wide_ragged_plain": dict(_S, critic_dims=(4000,), policy_dims=(64,), critic_layer_norm=False, rows=2, rates=(0.1, 0.1)),
    "image_only": dict(image_keys=("wrist",), H=32, W=32, encoder_type="small", S=5, A=3, ensemble=2, subsample=None, use_proprio=False,
                       critic_dims=(64, 64), policy_dims=(64, 64), rows=6, rates=(0.1, 0.1)),
}


def calls_of(name):
    """update_critics and one update_high_utd whose UTD divides the rows: 5 at 65 rows, 2 at 6 and 2, 1 at one row"""
    rows = CASES[name]["rows"]
    return ["critics", ("high_utd", 5 if rows % 5 == 0 else 2 - rows % 2)]


def case_config(name):
    """-> (ImageOnlyConfig, rows, rates, kink)"""
    c = dict(CASES[name])
    rows, rates, kink = c.pop("rows"), c.pop("rates"), c.pop("kink", False)
    return IO.ImageOnlyConfig(hidden=c["critic_dims"][0], **c), rows, rates, kink


def random_masks(cfg, rates, kind, n_critic, rows, seed):
    """{site: [u8[rows, d_l] per layer]} of a call, every site that draws at these rates"""
    rng = np.random.default_rng(seed)
    dims = dict(zip(("critic", "policy"), MS.dims_of(cfg)))
    rate = {"critic": rates[0], "policy": rates[1]}
    want = {s for s, _ in MD.site_order(kind, n_critic)} & set(MD.sites_of(rates))
    return {s: [(rng.random((rows, d)) < 1.0 - rate[MLP_SITE_NETWORK[s]]).astype(np.uint8) for d in dims[MLP_SITE_NETWORK[s]]]
            for s in MD.MLP_SITES if s in want}


def device_noise(masks):
    return {"drop_mask_" + s: [torch.tensor(m, device="cuda") for m in ms] for s, ms in masks.items()}


_HOOK = []      # the active (rate by network, queue of (site, layer, mask), seen) of oracle_dropout


def _drop(net, layer, x):
    if not _HOOK or not _HOOK[-1][0][net] > 0:
        return x
    rate, queue, seen = _HOOK[-1]
    site, l, m = queue.pop(0)
    assert (MLP_SITE_NETWORK[site], l) == (net, layer) and tuple(m.shape) == tuple(x.shape[-2:]), (site, l, net, layer, m.shape, x.shape)
    x = x * (torch.as_tensor(m, dtype=x.dtype) / (1.0 - rate[net]))      # [E, rows, d] * [rows, d]: one mask for every member
    seen.append((site, layer, x.detach()))
    return x


def policy_mlp(th, cfg, enc):
    ln, h = MP.layer_norms_of(cfg)[1], enc
    for j in range(1, len(MS.dims_of(cfg)[1]) + 1):
        h = _drop("policy", j - 1, h @ th[f"actor/w{j}"] + th[f"actor/b{j}"])
        if ln:
            h = O.layer_norm(h, th[f"actor/ln{j}/scale"], th[f"actor/ln{j}/bias"])
        h = MP._act("policy", cfg, h)
    return h


def critic_forward(th, cfg, enc, act):
    ln, h = MP.layer_norms_of(cfg)[0], torch.cat([enc, act], dim=-1)
    for j in range(1, len(MS.dims_of(cfg)[0]) + 1):
        h = torch.einsum("bi,eio->ebo" if j == 1 else "ebi,eio->ebo", h, th[f"critic/w{j}"]) + th[f"critic/b{j}"][:, None, :]
        h = _drop("critic", j - 1, h)
        if ln:
            h = O.layer_norm(h, th[f"critic/ln{j}/scale"][:, None, :], th[f"critic/ln{j}/bias"][:, None, :])
        h = MP._act("critic", cfg, h)
    if cfg.state_only:
        return torch.einsum("ebi,eio->ebo", h, th["critic/head/kernel"]).squeeze(-1) + th["critic/head/bias"][:, None]
    return (h @ th["critic/head/kernel"]).squeeze(-1) + th["critic/head/bias"]


@contextlib.contextmanager
def installed():
    """tests/image_only.py's general oracle with the two forward functions above"""
    with IO.installed():
        O.policy_mlp, O.critic_forward = policy_mlp, critic_forward
        yield


@contextlib.contextmanager
def oracle_dropout(rates, masks, kind, n_critic, rows):
    """for the duration the oracle's six MLP evaluations apply `masks` in the reference's draw order (critic update i reads rows
    [i * mb, (i + 1) * mb)); the queue must be used up.  -> the (site, layer, masked input) of every evaluation"""
    mb, queue, seen = rows // max(n_critic, 1), [], []
    for site, i in MD.site_order(kind, n_critic):
        if site in masks:
            queue += [(site, l, m if i is None else m[i * mb:(i + 1) * mb]) for l, m in enumerate(masks[site])]
    _HOOK.append(({"critic": rates[0], "policy": rates[1]}, queue, seen))
    try:
        yield seen
        assert not queue, f"{len(queue)} masks were not used"
    finally:
        _HOOK.pop()


def init_params(cfg, seed, kink):
    trunk, theta = IO.init_params(cfg, seed)
    if not kink:
        return trunk, theta
    # (kink_margin sets the LayerNorm vectors of two layers in both networks: a network without them lends it stand-ins)
    lent = {f"{net}/{ln}/{p}": np.zeros((1, 8), np.float32) for net in ("critic", "actor") for ln in ("ln1", "ln2") for p in ("scale", "bias")
            if f"{net}/{ln}/{p}" not in theta}
    out = MA.kink_margin({**theta, **lent})
    return trunk, {k: out[k] for k in theta}


def make_core(cfg, B, rates, leaves=None, *, fuse=None, dropout_any=True):
    """tests/image_only.py's make_core with the two rates, wide_widths where a width is above 1024 and the switch"""
    import serl_amd.agents.core as core_mod
    orig = core_mod.AgentCore
    wide = max(cfg.critic_dims + cfg.policy_dims) > 1024
    core_mod.AgentCore = functools.partial(orig, critic_dropout=rates[0], policy_dropout=rates[1], wide=wide, dropout_any=dropout_any)
    try:
        core = IO.make_core(cfg, B, fuse=fuse)
    finally:
        core_mod.AgentCore = orig
    return core if leaves is None else AH.load_leaves(core, cfg, *leaves)


_RUNS = {}


def oracle_run(name, call, seed=42):
    """one call of the case in fp64 with random masks: computed once, inside installed(), unchanged by its readers"""
    if (name, call) not in _RUNS:
        cfg, B, rates, kink = case_config(name)
        leaves = init_params(cfg, seed, kink)
        st, utd, d = O.TrainState(cfg, *leaves, torch.float64), 1 if call == "critics" else call[1], call != "critics"
        kind = "high_utd" if d else "critics"
        if (name, call) == ("wide_one_row", "critics"):      # row 0 of the 65-row case: batch, noise and masks
            src = oracle_run("wide", call)
            row0 = lambda v: v[:1] if isinstance(v, np.ndarray) and v.shape[:1] == (src["B"],) else v      # noqa: E731
            b, noise = ({k: row0(v) for k, v in src[w].items()} for w in ("batch", "noise"))
            masks = {s: [m[:1] for m in ms] for s, ms in src["masks"].items()}
        else:
            b, noise = AH.synth_batch(cfg, B, seed=3 + d), O.make_noise(cfg, B, seed=7 + d, utd_ratio=utd)
            masks = random_masks(cfg, rates, kind, utd, B, seed=11 + d)
        with oracle_dropout(rates, masks, kind, utd, B), MP.relu_margin() as rec:
            tb, tn = AH.batch_to_torch(b, torch.float64), O.noise_to_torch(noise, torch.float64)
            info, aux = O.update_high_utd(st, tb, tn, utd) if d else O.update_critics(st, tb, tn)
        _RUNS[name, call] = dict(cfg=cfg, B=B, rates=rates, leaves=init_params(cfg, seed, kink), batch=b, noise=noise, masks=masks, state=st,
                                 info=info, aux=aux, relu=list(rec))
    return _RUNS[name, call]
