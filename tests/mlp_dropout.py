"""Shared by the tests of Dropout in the critic's and the policy's MLP (networks/mlp.py:27-28: Dense -> Dropout -> LayerNorm ->
activation in both hidden layers; DroQ is the critic's): the fixture table of tests/golden/drop_*.npz
(tests/golden/make_golden_update_dropout.py), the order in which an update call draws its MLP masks, their packing, and the fp64
statement of the update with the masks applied -- the oracle's own update functions, with O.layer_norm wrapped at run time so that
the four LayerNorms of an MLP evaluation multiply their input by the next mask first.

A call's masks are {site: u8[2 layers, rows, hidden]} over serl_amd._lib_agent.MLP_SITES; the critic-loss sites of a call with n
critic updates hold update i in rows [i * mb, (i + 1) * mb).  One mask serves every ensemble member: the reference's vmapped critic
splits only its params stream."""
import contextlib
import dataclasses

import numpy as np
import torch

from oracle import drq_oracle as O
from oracle import ref_update_runner as RR
from serl_amd._lib_agent import MLP_CRITIC_LOSS_SITES, MLP_SITE_NETWORK, MLP_SITES
import golden_replay as GR

CRITIC_STEP = ("pi_next", "q_target", "q_online")      # draw order inside critic_loss_fn (sac.py:137-176)
ACTOR, TEMP = ("pi", "q_actor"), ("pi_temp",)           # policy_loss_fn (sac.py:197-207), temperature_loss_fn (sac.py:222-227)
def standin_dropout_path(network, layer, state_only=True):
    """The Dropout scope paths under the stand-in flax of oracle/jaxshim.  The policy's is the library's
    (jaxrng.mlp_dropout_path).  The critic's vmapped members are bound at a fresh root there, so the path starts below the vmap:
    at the Critic's `network` field for state-only SAC (ensemblize wraps the whole Critic), at the MLP itself for DrQ (ensemblize
    wraps the MLP) -- flax's own rule keeps the path from the root."""
    if network == "policy":
        return ("modules_actor", "network", f"Dropout_{layer}")
    return ("network", f"Dropout_{layer}") if state_only else (f"Dropout_{layer}",)


def _row(rates, rows, sched, n_sample=512, **kw):
    return dict(cfg=O.Config(**kw), B=rows, sched=sched, rates=rates, n_sample=n_sample)


# name -> the run: oracle Config, rows, schedule, (critic rate, policy rate), sampled elements per large leaf
GOLDEN = {
    "update_sac_state": _row((0.1, 0.05), 72, GR.STATE_SCHED, warmup=2000, **GR.STATE),
    "update_sac_state_droq": _row((0.01, 0.0), 72, GR.STATE_SCHED, warmup=2000, ensemble=2, subsample=None, **GR.STATE),
    "update_sac_state_w320_swish": _row((0.1, 0.1), 72, GR.STATE_SCHED, 256, warmup=2000, ensemble=5, hidden=320, critic_activation="swish",
                                        policy_activation="swish", **GR.STATE),
    "update_drq_one_cam": _row((0.1, 0.05), 6, [("critics",), ("high_utd", 2)], image_keys=("image",), H=64, W=64, S=5, A=3),
}


def network_kwargs(cfg, which, rate):
    """the launcher's critic_network_kwargs / policy_network_kwargs at the Config's width and activation, with a dropout_rate"""
    act = cfg.critic_activation if which == "critic" else cfg.policy_activation
    return {"activations": act, "use_layer_norm": True, "hidden_dims": [cfg.hidden, cfg.hidden], "dropout_rate": rate}


def site_order(kind, n_critic, nets=()):
    """[(site, critic update or None)] in the order the reference's losses draw (loss names sorted: actor, critic, temperature)"""
    crit = [(s, i) for i in range(n_critic) for s in CRITIC_STEP]
    if kind == "critics":
        return crit
    if kind == "high_utd":
        return crit + [(s, None) for s in ACTOR + TEMP]
    out = [(s, None) for s in ACTOR] if "actor" in nets else []
    out += crit if "critic" in nets else []
    return out + ([(s, None) for s in TEMP] if "temperature" in nets else [])


def sites_of(rates):
    """the sites that draw at (critic rate, policy rate)"""
    r = {"critic": rates[0], "policy": rates[1]}
    return [s for s in MLP_SITES if r[MLP_SITE_NETWORK[s]] > 0]


def step_shape(step):
    """(kind, number of critic updates, nets) of a golden's step"""
    kind = step["kind"]
    return kind, (step["utd"] if kind == "high_utd" else (1 if kind == "critics" or "critic" in step["nets"] else 0)), step["nets"]


def pack(masks):
    """{site: u8[2, rows, h]} -> {"drop_<site>": packed bits}"""
    return {"drop_" + s: np.packbits(m.astype(np.uint8), axis=None) for s, m in masks.items()}


def unpack(noise, rows, hidden):
    """the "drop_<site>" entries of a step's unpacked noise -> {site: u8[2, rows, h]}"""
    return {k[5:]: np.unpackbits(np.asarray(v))[:2 * rows * hidden].reshape(2, rows, hidden) for k, v in noise.items() if k.startswith("drop_")}


def random_masks(rates, kind, n_critic, nets, rows, hidden, seed):
    """test masks of a call, every site that draws at these rates"""
    rng = np.random.default_rng(seed)
    r = {"critic": rates[0], "policy": rates[1]}
    want = {s for s, _ in site_order(kind, n_critic, nets)} & set(sites_of(rates))
    return {s: (rng.random((2, rows, hidden)) < 1.0 - r[MLP_SITE_NETWORK[s]]).astype(np.uint8) for s in MLP_SITES if s in want}


def device_noise(masks):
    """{site: u8[2, rows, h]} -> the entries of an update's `noise` dict (AgentCore._noise)"""
    return {"drop_mask_" + s: torch.tensor(m, device="cuda") for s, m in masks.items()}


@contextlib.contextmanager
def oracle_dropout(rates, queue):
    """For the duration, the oracle's MLPs are the reference's with Dropout: inside O.policy_mlp / O.critic_forward every
    O.layer_norm first replaces its input x by where(mask, x / keep, 0) with the next mask of `queue`, a list of (site, layer,
    mask [rows, h] as a bool or 0/1 array); a network at rate 0 takes nothing.  The list must be used up by the end.  `seen`
    (yielded) collects (site, layer, the masked input) of every evaluation."""
    rate = {"critic": rates[0], "policy": rates[1]}
    state = {"net": None}
    queue, seen = list(queue), []
    ln, pm, cf = O.layer_norm, O.policy_mlp, O.critic_forward

    def layer_norm(x, scale, bias, eps=1e-6):
        net = state["net"]
        if net is not None and rate[net] > 0:
            site, layer, m = queue.pop(0)
            assert MLP_SITE_NETWORK[site] == net, (site, net)
            m = torch.as_tensor(np.asarray(m), dtype=x.dtype)
            assert tuple(m.shape) == tuple(x.shape[-2:]), (site, layer, m.shape, x.shape)
            x = x * (m / (1.0 - rate[net]))      # [E, rows, h] * [rows, h]: one mask for every member
            seen.append((site, layer, x.detach()))
        return ln(x, scale, bias, eps)

    def within(net, fn):
        def run(*a, **k):
            state["net"] = net
            try:
                return fn(*a, **k)
            finally:
                state["net"] = None
        return run
    O.layer_norm, O.policy_mlp, O.critic_forward = layer_norm, within("policy", pm), within("critic", cf)
    try:
        yield seen
        assert not queue, f"{len(queue)} masks were not used"
    finally:
        O.layer_norm, O.policy_mlp, O.critic_forward = ln, pm, cf


def mask_queue(masks, rates, kind, n_critic, nets, rows):
    """the masks of one call in the order the oracle's update evaluates its MLPs -- the reference's draw order"""
    drawing, out = set(sites_of(rates)), []
    mb = rows // max(n_critic, 1)
    order = site_order(kind, n_critic, nets)
    if kind == "update":      # (O.update evaluates its critic loss first; which mask a site gets does not depend on the order)
        order = sorted(order, key=lambda si: si[1] is None)
    for site, i in order:
        if site in drawing:
            m = masks[site] if i is None else masks[site][:, i * mb:(i + 1) * mb]
            out += [(site, 0, m[0]), (site, 1, m[1])]
    return out


def run_steps(st, steps, rates, dtype=torch.float64, on_info=None):
    """RR.run_steps with each step's recorded MLP masks applied"""
    cfg = st.cfg
    infos = []
    for i, step in enumerate(steps):
        kind, n_critic, nets = step_shape(step)
        B = step["batch"]["reward"].shape[0]
        masks = unpack(step["noise"], B, cfg.hidden)
        plain = dict(step, noise={k: v for k, v in step["noise"].items() if not k.startswith("drop_")})
        with oracle_dropout(rates, mask_queue(masks, rates, kind, n_critic, nets, B)):
            (info,) = RR.run_steps(st, [plain], dtype, on_info=None if on_info is None else (lambda _, s, inf, i=i: on_info(i, s, inf)))
        infos.append(info)
    return infos


def launcher_cfg(cfg):
    """the Config the reference's run is given: activations reach it through the factories' kwargs"""
    return dataclasses.replace(cfg, critic_activation="tanh", policy_activation="tanh")


class Injecting:
    """An agent whose update calls add the recorded MLP masks of schedule item i to the injected noise: golden_replay.replay then
    drives a Dropout agent like any other (the masks go through the `noise=` hook of the update methods)."""

    def __init__(self, agent, steps, hidden):
        self.__dict__.update(_agent=agent, _steps=steps, _hidden=hidden, _i=0)

    def __getattr__(self, name):
        return getattr(self._agent, name)

    def _call(self, method, batch, kw):
        step = self._steps[self._i]
        self.__dict__["_i"] += 1
        if kw.get("noise") is not None:
            B = step["batch"]["reward"].shape[0]
            kw["noise"] = {**kw["noise"], **device_noise(unpack(step["noise"], B, self._hidden))}
        _, info = getattr(self._agent, method)(batch, **kw)
        return self, info

    def update_critics(self, batch, **kw):
        return self._call("update_critics", batch, kw)

    def update_high_utd(self, batch, **kw):
        return self._call("update_high_utd", batch, kw)

    def update(self, batch, **kw):
        return self._call("update", batch, kw)
