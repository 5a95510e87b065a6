"""Shared by tests/test_policy_modes_cpu.py, tests/test_policy_modes_gpu.py and tests/golden/make_golden_update_policy.py: the
policy distributions beside the launcher's (std_parameterization "exp" / "softplus" / "uniform" x tanh_squash_distribution True /
False; the std_param / no_tanh arguments of serl_agent_create_policy), the table of the policy_*.npz fixtures, the parameters each fixture's run starts from,
and a float64 restatement of the policy head (actor_critic_nets.py:189-227, distrax MultivariateNormalDiag [+ Tanh])."""
import math

import numpy as np
import torch

from oracle import drq_oracle as O
import agent_helpers as AH
import golden_replay as GR
import trained_regime as TR

LOG_STDS_SEED = 17

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

# name -> (oracle Config, rows, schedule, (std, squash), regime, sampled elements per large leaf).  State-only: golden_replay's
# shared shape.  The pixel case is create_drq's own default pair.
GOLDEN = {
    "update_sac_state_softplus": (O.Config(warmup=2000, **GR.STATE), 72, GR.STATE_SCHED, ("softplus", True), "init", 1024),
    "update_sac_state_gauss": (O.Config(warmup=2000, **GR.STATE), 72, GR.STATE_SCHED, ("exp", False), "init", 1024),
    "update_sac_state_uniform": (O.Config(warmup=2000, **GR.STATE), 72, GR.STATE_SCHED, ("uniform", True), "init", 1024),
    "update_sac_state_uniform_gauss": (O.Config(warmup=2000, **GR.STATE), 72, GR.STATE_SCHED, ("uniform", False), "init", 1024),
    "update_drq_uniform": (O.Config(image_keys=("image",), H=64, W=64, S=5, A=3), 6, [("critics",), ("high_utd", 2)],
                           ("uniform", True), "init", 1024),
    "trained_sac_state_softplus": (O.Config(warmup=4, **GR.STATE), 72, GR.STATE_SCHED, ("softplus", True), "trained", 1024),
    "trained_sac_state_uniform": (O.Config(warmup=4, **GR.STATE), 72, GR.STATE_SCHED, ("uniform", True), "trained", 1024),
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


def initial_leaves(name):
    """-> (trunk, theta) the run of fixture `name` started from, oracle names"""
    cfg, _, _, (std, _), regime, _ = GOLDEN[name]
    return GR.initial_leaves(cfg, lambda theta, c: mode_theta(theta, c, std, regime))


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
