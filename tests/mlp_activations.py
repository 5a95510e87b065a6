"""Shared by tests/test_mlp_activations_cpu.py, tests/test_mlp_activations_gpu.py and tests/golden/make_golden_update_activations.py:
the activations of the critic's and the policy's MLP beside the launcher's tanh (networks/mlp.py:19-31; the critic_act / policy_act
arguments of serl_agent_create_mlp), the table of the act_*.npz fixtures, the parameters each fixture's run starts from, and the
Recorder of pre-activations behind the relu kink condition.  The activations themselves are stated in oracle/drq_oracle.py
(Config.critic_activation / policy_activation, ACTIVATIONS); a Recorder sees them through O.observe_preactivations."""
import numpy as np
import torch

from oracle import drq_oracle as O
import golden_replay as GR
import trained_regime as TR

KINK_MIN = 1e-4        # the smallest |pre-activation| a relu comparison may contain (see `Recorder`)
KINK_SEEDS = 10

NEW_ACTS = ("swish", "relu")


def network_kwargs(act, h=256):
    """the launcher's critic_network_kwargs / policy_network_kwargs (utils/launcher.py:50-116) with another activation"""
    return {"activations": act, "use_layer_norm": True, "hidden_dims": [h, h]}


def _row(critic, policy, rows, sched, regime, **kw):
    return O.Config(critic_activation=critic, policy_activation=policy, **kw), rows, sched, (critic, policy), regime, 1024


# name -> (oracle Config, rows, schedule, (critic activation, policy activation), regime, sampled elements per large leaf).  The
# Config carries the activations; the pair repeats them for the check against a file's meta block.  State-only: golden_replay's
# shared shape.
GOLDEN = {
    "update_sac_state_swish": _row("swish", "swish", 72, GR.STATE_SCHED, "init", warmup=2000, **GR.STATE),
    "update_sac_state_relu": _row("relu", "relu", 72, GR.STATE_SCHED, "kink_margin", warmup=2000, **GR.STATE),
    "update_sac_state_mixed": _row("relu", "swish", 72, GR.STATE_SCHED, "kink_margin", warmup=2000, **GR.STATE),
    "trained_sac_state_swish": _row("swish", "swish", 72, GR.STATE_SCHED, "trained", warmup=4, **GR.STATE),
    "update_drq_swish": _row("swish", "swish", 6, [("critics",), ("high_utd", 2)], "init", image_keys=("image",), H=64, W=64, S=5, A=3),
}


MARGIN_SEED = 23
SAFE_SCALE, SAFE_BIAS, LIVE_BIAS, SAFE_REACH = 0.05, 1.0, 0.3, 0.8


def safe_scale(D):
    """the LayerNorm scale of a safe column at width D: |scale * xhat| <= SAFE_REACH = 0.8 < SAFE_BIAS whatever the row, since
    |xhat| <= sqrt(D - 1).  SAFE_SCALE = 0.05 up to width 257 (0.05 sqrt(255) = 0.798), 0.8 / sqrt(D - 1) above (0.025 at 1024)."""
    return min(SAFE_SCALE, SAFE_REACH / float(np.sqrt(D - 1)))


GOLDEN_LIVE = 4      # live columns per LayerNorm vector in the relu fixtures


def kink_margin(theta, seed=MARGIN_SEED, n_live=GOLDEN_LIVE):
    """LayerNorm leaves of the four MLP layers under which a run CAN keep every relu pre-activation KINK_MIN away from 0.  With
    O.init_params' leaves (scale ~ 1, bias ~ 0) a pre-activation has density 0.4 at 0 and a run of the fixtures' schedule evaluates
    8e6 of them: the smallest is 1e-7 whatever the batch seed.  Here every LayerNorm vector (every member's, in the critic) keeps
    n_live live columns -- scale 1, bias LIVE_BIAS: the sign changes from row to row, the unit is off in about 40 % of the rows --
    and all other columns are safe: scale safe_scale(D), bias +-SAFE_BIAS by a seeded coin, so |pre| >= 0.2 in every row: on in
    every row, or off in every row (output and gradient exactly 0).  Only the live pre-activations can come near 0, and there are
    few enough of them (1.4e5 in a fixture's run with GOLDEN_LIVE = 4 live columns) for a batch seed to keep them all KINK_MIN
    away: with ONE live column 19 (relu) and 18 (mixed) of the batch seeds 100, 116, ..., 564 did; what the generator found with
    four is in each file's meta (batch_seed, seeds_tried)."""
    rng = np.random.default_rng(seed)
    out = {k: np.array(v, np.float32) for k, v in theta.items()}
    for net in ("critic", "actor"):
        for ln in ("ln1", "ln2"):
            sc, bi = out[f"{net}/{ln}/scale"], out[f"{net}/{ln}/bias"]
            D = sc.shape[-1]
            rows_sc, rows_bi = sc.reshape(-1, D), bi.reshape(-1, D)     # (views: one row per member)
            for r in range(rows_sc.shape[0]):
                live = rng.choice(D, size=n_live, replace=False)
                rows_sc[r, :] = safe_scale(D)
                rows_bi[r, :] = np.where(rng.random(D) < 0.5, SAFE_BIAS, -SAFE_BIAS)
                rows_sc[r, live], rows_bi[r, live] = 1.0, LIVE_BIAS
    return out


def act_theta(theta, cfg, regime):
    """O.init_params' leaves -> the leaves a fixture's run starts from (oracle names), float32.  "trained": trained_regime.trained_like
    (lagrange 0.5): LayerNorm scales up to 3 in front of the activation.  "kink_margin": kink_margin above (the relu fixtures)."""
    if regime == "trained":
        return TR.trained_like(theta, cfg, lam=0.5)
    if regime == "kink_margin":
        return kink_margin(theta)
    assert regime == "init", regime
    return {k: np.array(v, np.float32) for k, v in theta.items()}


def initial_leaves(name):
    """-> (trunk, theta) the run of fixture `name` started from, oracle names"""
    cfg, _, _, _, regime, _ = GOLDEN[name]
    return GR.initial_leaves(cfg, lambda theta, c: act_theta(theta, c, regime))


class Kink(Exception):
    """a pre-activation closer to 0 than a Recorder's floor; args[0] = its absolute value"""


class Recorder:
    """What an activation saw: per evaluation (one call) the smallest and the largest |pre-activation|.  ReLU's kink: an fp32 run
    may put a pre-activation on the other side of 0 than the fp64 one, which flips a gradient term; a relu comparison counts only
    where every evaluation stayed KINK_MIN away from 0 -- a condition on the inputs, checked on the fp64 side alone."""

    def __init__(self, floor=None):
        """floor: raise Kink at the first evaluation that comes closer to 0 (a seed search need not finish a run that is out)"""
        self.floor = floor
        self.reset()

    def reset(self):
        self.min_abs, self.max_abs, self._off, self._live = [], [], 0, 0

    @property
    def off_fraction(self):
        """over the columns whose sign differed between the rows of an evaluation: the fraction of entries below 0"""
        return self._off / self._live if self._live else None

    def see(self, x):
        rows = x.shape[-2] if x.dim() > 1 else 1      # (a factory's init pass hands over one observation)
        neg = (x.detach().reshape(-1, rows, x.shape[-1]) < 0).to(torch.float64)      # [member, row, column]
        mixed = (neg.mean(1) > 0) & (neg.mean(1) < 1)
        self._off += int((neg * mixed[:, None, :]).sum())
        self._live += int(mixed.sum()) * neg.shape[1]
        a = x.detach().abs()
        self.min_abs.append(float(a.min()))
        self.max_abs.append(float(a.max()))
        if self.floor is not None and self.min_abs[-1] < self.floor:
            raise Kink(self.min_abs[-1])

    @property
    def kink_free(self):
        return bool(self.min_abs) and min(self.min_abs) >= KINK_MIN
