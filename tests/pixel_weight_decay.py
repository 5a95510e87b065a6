"""Shared by tests/test_pixel_weight_decay_cpu.py, tests/test_pixel_weight_decay_gpu.py and
tests/golden/make_golden_update_decay.py: weight_decay in the optimizer kwargs of an agent with cameras.

optax.adamw decays every leaf of the tree it is given (common/optimizers.py:39-42), and the reference gives it the whole parameter
tree, the pretrained ResNet-10 included.  With a decay on, every optimizer step multiplies every trunk leaf by
1 - sum_t lr_t * wd_t (all three optimizers step on every update) and the target copy follows by the EMA on critic
steps only: the two trunks differ from the second step on.  oracle/drq_oracle.py states all of it (apply_gradients,
target_update, and TrainState.live_trunk: features of the trunks as they are at each step, the target critic on the target copy).
This module holds the table of the wd_*.npz fixtures (the reference's own DrQAgent under oracle/jaxshim, recorded by the
generator) and the closed form a decayed trunk leaf follows.
"""
import numpy as np
import torch

from oracle import drq_oracle as O

# decay 20 / 30 / 10 at lr 3e-4: each optimizer step multiplies the trunk by 1 - 3e-4 * 60 = 0.982
DECAY = {"actor": 20.0, "critic": 30.0, "temperature": 10.0}
OPT = {tx: {"weight_decay": wd} for tx, wd in DECAY.items()}
ONE_CAM = dict(image_keys=("image",), H=64, W=64, S=5, A=3)
SCHED = [("critics",), ("high_utd", 2), ("critics",)]      # five optimizer steps, four of them with the EMA
# three steps: 0.982^3 = 0.947, so that this fixture too moves every trunk leaf by more than 5 %; both forms of SACAgent.update
SCHED_UPDATE = [("update", ("actor", "critic", "temperature")), ("update", ("critic",)), ("update", ("actor", "critic", "temperature"))]

# name -> (oracle Config, rows, schedule, sampled elements per large leaf).  6 rows: high_utd 2 runs 3-row minibatches.  768 samples
# (recorded in each file as wd_n_sample): with the two conv_init copies beside them a file stays clear of 1 MiB.
GOLDEN = {
    "update_drq_one_cam": (O.Config(opt=OPT, **ONE_CAM), 6, SCHED, 768),
    "update_drq_small": (O.Config(opt=OPT, encoder_type="small", **ONE_CAM), 6, SCHED, 768),
    "update_sac_pixels_update": (O.Config(opt=OPT, **ONE_CAM), 6, SCHED_UPDATE, 768),
}
PRETRAINED = [n for n, c in GOLDEN.items() if not c[0].small]

# every option beside the launcher's at once, which no recorded run covers: softplus std (squashed), swish in both MLPs, the decay
# above on a pretrained trunk.  6 rows as the fixtures: update_high_utd(2) runs 3-row minibatches.
COMPOSED = O.Config(opt=OPT, std_parameterization="softplus", tanh_squash=True, critic_activation="swish", policy_activation="swish",
                    **ONE_CAM)
COMPOSED_ROWS = 6


def optimizer_steps(schedule):
    """-> [True where the step runs the target EMA] over the optimizer steps of a schedule, in order"""
    out = []
    for item in schedule:
        if item[0] == "critics":
            out += [True]
        elif item[0] == "high_utd":
            out += [True] * item[1] + [False]
        else:
            out += ["critic" in item[1]]
    return out


def step_factor(cfg):
    """what one optimizer step multiplies a trunk leaf by, as O.apply_gradients forms it: the learning rates enter as float32
    (optax.inject_hyperparams), the three terms are added in the optimizers' dict order"""
    st = O.TrainState(cfg, {}, {}, torch.float64)
    decay = 0.0
    for tx in O.TX_NAMES:
        wd = st.tx_opt(tx)["weight_decay"]
        if wd is not None:
            decay += float(np.float32(st.lr_at(0, tx))) * wd      # (constant schedules in every fixture)
    return 1.0 - decay


def closed_form_ratios(cfg, schedule):
    """-> (online, target): what a trunk element ends at, relative to its start, after the schedule"""
    f, p, t = step_factor(cfg), 1.0, 1.0
    for ema in optimizer_steps(schedule):
        p = p * f
        if ema:
            t = p * cfg.tau + t * (1.0 - cfg.tau)
    return p, t
