"""Shared by tests/test_policy_modes_cpu.py, tests/test_policy_modes_gpu.py and tests/golden/make_golden_update_policy.py: the
policy distributions beside the launcher's (std_parameterization "exp" / "softplus" / "uniform" x tanh_squash_distribution True /
False; the std_param / no_tanh arguments of serl_agent_create_policy), the table of the policy_*.npz fixtures, the parameters each fixture's run starts from,
and a float64 restatement of the policy head (actor_critic_nets.py:189-227, distrax MultivariateNormalDiag [+ Tanh])."""
import json
import math
import os

import numpy as np
import torch

from oracle import drq_oracle as O
from oracle import golden_update as G
import agent_helpers as AH
import trained_regime as TR

GOLDEN_DIR = os.path.join(os.path.dirname(__file__), "golden")
PARAM_SEED, BATCH_SEED, LOG_STDS_SEED = 42, 100, 17

# (std_parameterization, tanh_squash_distribution); the first is what utils/launcher.py writes down and every other test runs
DEFAULT_MODE = ("exp", True)
NEW_MODES = [("softplus", True), ("uniform", True), ("exp", False), ("softplus", False), ("uniform", False)]
MODE_IDS = [f"{s}{'' if t else '_gauss'}" for s, t in NEW_MODES]


def policy_kwargs(std, squash):
    """the launcher's policy_kwargs (utils/launcher.py:55-60) with another distribution"""
    return {"tanh_squash_distribution": squash, "std_parameterization": std, "std_min": 1e-5, "std_max": 5}


# log-std bias / log_stds per action column j % 4 of the trained-regime fixtures: exp(-14) = 8e-7 and softplus(-14) = 8e-7 lie below
# std_min = 1e-5; exp(7) = 1097 and softplus(7) = 7.0009 lie above std_max = 5; exp / softplus of -3 and 0.5 lie inside.  (The +3 of
# trained_regime.LOGSTD_CYCLE clips exp(3) = 20 but not softplus(3) = 3.05.)  The log-std kernel of trained_like moves a row's value
# by a few tenths: the bias decides.
CLIP_CYCLE = (-14.0, -3.0, 0.5, 7.0)

_STATE = dict(image_keys=(), S=10, A=5, discount=0.99, temp_warmup=0)
_STATE_SCHED = [("high_utd", 2), ("update", ("actor", "critic", "temperature")), ("high_utd", 1)]
# name -> (oracle Config, rows, schedule, (std, squash), regime, sampled elements per large leaf).  State-only: B = 72 = two 64-row
# head tiles, the second ragged, divisible by the UTD; A = 5 is odd.  The pixel case is create_drq's own default pair.
GOLDEN = {
    "update_sac_state_softplus": (O.Config(warmup=2000, **_STATE), 72, _STATE_SCHED, ("softplus", True), "init", 1024),
    "update_sac_state_gauss": (O.Config(warmup=2000, **_STATE), 72, _STATE_SCHED, ("exp", False), "init", 1024),
    "update_sac_state_uniform": (O.Config(warmup=2000, **_STATE), 72, _STATE_SCHED, ("uniform", True), "init", 1024),
    "update_sac_state_uniform_gauss": (O.Config(warmup=2000, **_STATE), 72, _STATE_SCHED, ("uniform", False), "init", 1024),
    "update_drq_uniform": (O.Config(image_keys=("image",), H=64, W=64, S=5, A=3), 6, [("critics",), ("high_utd", 2)],
                           ("uniform", True), "init", 1024),
    "trained_sac_state_softplus": (O.Config(warmup=4, **_STATE), 72, _STATE_SCHED, ("softplus", True), "trained", 1024),
    "trained_sac_state_uniform": (O.Config(warmup=4, **_STATE), 72, _STATE_SCHED, ("uniform", True), "trained", 1024),
}
STD_DENSE = ("actor/logstd/kernel", "actor/logstd/bias")


def mode_theta(theta, cfg, std, regime):
    """O.init_params' leaves -> the leaves a fixture's run starts from (oracle names), float32.  "trained": trained_regime.trained_like
    (lagrange 0.5) with CLIP_CYCLE on the log-std bias.  "uniform": no log-std Dense; actor/log_stds = CLIP_CYCLE ("trained"), or
    seeded values in [-1.5, 0.5) ("init": the reference's zeros would leave std = 1 in every column)."""
    out = {k: np.array(v, np.float32) for k, v in theta.items()}
    cyc = np.array([CLIP_CYCLE[j % 4] for j in range(cfg.A)], np.float32)
    if regime == "trained":
        out = TR.trained_like(out, cfg, lam=0.5)
        out["actor/logstd/bias"] = cyc
    else:
        assert regime == "init", regime
    if std == "uniform":
        for k in STD_DENSE:
            del out[k]
        out["actor/log_stds"] = cyc if regime == "trained" else \
            np.random.default_rng(LOG_STDS_SEED).uniform(-1.5, 0.5, cfg.A).astype(np.float32)
    return out


def leaf_names(cfg, std):
    """the trainable leaves (oracle names) of an agent with this std parameterisation, in arena order"""
    names = [k for k in O.trainable_param_shapes(cfg)]
    if std == "uniform":
        i = names.index(STD_DENSE[0])
        names[i:i + 2] = ["actor/log_stds"]
    return names


def flax_paths(cfg, std):
    """oracle leaf name -> flax path, from the product's mapping (what oracle.ref_update_runner.theta_flax_paths does for "exp")"""
    from serl_amd.agents.flax_tree import theta_paths
    prod = theta_paths(cfg.image_keys, encoder_type=cfg.encoder_type, std_parameterization=std)
    return {k: prod[AH.product_name(k, cfg.image_keys)][0] for k in leaf_names(cfg, std)}


def golden_path(name):
    return os.path.join(GOLDEN_DIR, f"policy_{name}.npz")


def load_golden(name, monkeypatch=None):
    """-> (G.unpack of tests/golden/policy_<name>.npz, its meta["policy"], the npz)"""
    z = np.load(golden_path(name))
    if monkeypatch is not None:
        monkeypatch.setattr(G, "N_SAMPLE", int(z["policy_n_sample"]))
    meta = json.loads(str(z["meta"]))
    return (G.unpack(z) if monkeypatch is not None else None), meta["policy"], z


def initial_leaves(name):
    """-> (trunk, theta) the run of fixture `name` started from, oracle names"""
    cfg, _, _, (std, _), regime, _ = GOLDEN[name]
    trunk, theta = O.init_params(cfg, PARAM_SEED)
    return trunk, mode_theta(theta, cfg, std, regime)


def tree_has(tree, path):
    for k in path:
        if not isinstance(tree, dict) or k not in tree:
            return False
        tree = tree[k]
    return True


# ---- float64 restatement of the head ------------------------------------------------------------------------------------------
def mlp_features(th, cfg, enc):
    """the policy's two LayerNorm + tanh layers -> h2"""
    h = torch.tanh(O.layer_norm(enc @ th["actor/w1"] + th["actor/b1"], th["actor/ln1/scale"], th["actor/ln1/bias"]))
    return torch.tanh(O.layer_norm(h @ th["actor/w2"] + th["actor/b2"], th["actor/ln2/scale"], th["actor/ln2/bias"]))


def head(th, cfg, enc, std):
    """-> (mean, clipped std) [B, A] in the dtype of th"""
    h = mlp_features(th, cfg, enc)
    mean = h @ th["actor/mean/kernel"] + th["actor/mean/bias"]
    if std == "uniform":
        raw = torch.exp(th["actor/log_stds"]).expand_as(mean)
    else:
        pre = h @ th["actor/logstd/kernel"] + th["actor/logstd/bias"]
        raw = torch.nn.functional.softplus(pre) if std == "softplus" else torch.exp(pre)
    return mean, torch.clamp(raw, cfg.std_min, cfg.std_max)


def sample_and_log_prob(mean, sd, eps, squash):
    """-> (action, log pi): a = tanh(u) or u, u = mean + sd eps; the tanh's log-determinant only when squashed"""
    u = mean + sd * eps
    lp = (-0.5 * eps * eps - torch.log(sd) - 0.5 * math.log(2.0 * math.pi)).sum(-1)
    if not squash:
        return u, lp
    return torch.tanh(u), lp - (2.0 * (math.log(2.0) - u - torch.nn.functional.softplus(-2.0 * u))).sum(-1)


def core_with(cfg, B, std, squash, theta, trunk=None, fuse=None, target=None):
    """AgentCore of this distribution holding `theta` (oracle names) in params and target_params.  fuse: None = the default
    chain, True / False = SERL_CHAIN_FUSE 1 / 0 (read when an agent is created)."""
    from serl_amd.agents.core import AgentCore
    old = os.environ.get("SERL_CHAIN_FUSE")
    try:
        if fuse is not None:
            os.environ["SERL_CHAIN_FUSE"] = "1" if fuse else "0"
        core = AgentCore(encoder_type=cfg.encoder_type, n_cam=cfg.n_cam, H=cfg.H, W=cfg.W, state_dim=cfg.S, act_dim=cfg.A, batch=B,
                         ensemble=cfg.ensemble, hidden=cfg.hidden, discount=cfg.discount, tau=cfg.tau, lr=cfg.lr,
                         warmup_steps=cfg.warmup, dropout=cfg.dropout, std_min=cfg.std_min, std_max=cfg.std_max,
                         target_entropy=cfg.target_entropy, seed=0,
                         temp_warmup_steps=-1 if cfg.temp_warmup is None else cfg.temp_warmup,
                         std_parameterization=std, tanh_squash_distribution=squash)
    finally:
        if old is None:
            os.environ.pop("SERL_CHAIN_FUSE", None)
        else:
            os.environ["SERL_CHAIN_FUSE"] = old
    for sec in ("params", "target_params"):
        core.load_flat(sec, trunk or {})
        core.load_flat(sec, {AH.product_name(k, cfg.image_keys): v for k, v in theta.items()})
    return core
