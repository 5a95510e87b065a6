"""Shared by tests/test_policy_modes_cpu.py, tests/test_policy_modes_gpu.py and tests/golden/make_golden_update_policy.py: the
policy distributions beside the launcher's (std_parameterization "exp" / "softplus" / "uniform" x tanh_squash_distribution True /
False; the std_param / no_tanh arguments of serl_agent_create_policy), the table of the policy_*.npz fixtures and the parameters each
fixture's run starts from.  The distributions themselves are stated in oracle/drq_oracle.py (Config.std_parameterization /
tanh_squash: policy_head, sample_and_log_prob, trainable_param_shapes)."""
import numpy as np

from oracle import drq_oracle as O
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

def mode_config(std, squash, **kw):
    return O.Config(std_parameterization=std, tanh_squash=squash, **kw)


def _row(std, squash, rows, sched, regime, **kw):
    return mode_config(std, squash, **kw), rows, sched, (std, squash), regime, 1024


# name -> (oracle Config, rows, schedule, (std, squash), regime, sampled elements per large leaf).  The Config carries the mode; the
# pair repeats it for the check against a file's meta block.  State-only: golden_replay's shared shape.  The pixel case is
# create_drq's own default pair.
GOLDEN = {
    "update_sac_state_softplus": _row("softplus", True, 72, GR.STATE_SCHED, "init", warmup=2000, **GR.STATE),
    "update_sac_state_gauss": _row("exp", False, 72, GR.STATE_SCHED, "init", warmup=2000, **GR.STATE),
    "update_sac_state_uniform": _row("uniform", True, 72, GR.STATE_SCHED, "init", warmup=2000, **GR.STATE),
    "update_sac_state_uniform_gauss": _row("uniform", False, 72, GR.STATE_SCHED, "init", warmup=2000, **GR.STATE),
    "update_drq_uniform": _row("uniform", True, 6, [("critics",), ("high_utd", 2)], "init", image_keys=("image",), H=64, W=64, S=5, A=3),
    "trained_sac_state_softplus": _row("softplus", True, 72, GR.STATE_SCHED, "trained", warmup=4, **GR.STATE),
    "trained_sac_state_uniform": _row("uniform", True, 72, GR.STATE_SCHED, "trained", warmup=4, **GR.STATE),
}
STD_DENSE = ("actor/logstd/kernel", "actor/logstd/bias")


def mode_theta(theta, cfg, std, regime):
    """O.init_params' leaves of the launcher's ("exp") policy -> the leaves a fixture's run starts from (oracle names), float32.  "trained": trained_regime.trained_like
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
