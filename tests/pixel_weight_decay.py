"""Shared by tests/test_pixel_weight_decay_cpu.py, tests/test_pixel_weight_decay_gpu.py and
tests/golden/make_golden_update_decay.py: weight_decay in the optimizer kwargs of an agent with cameras.

optax.adamw decays every leaf of the tree it is given (common/optimizers.py:39-42), and the reference gives it the whole parameter
tree, the pretrained ResNet-10 included.  With a decay on, every optimizer step multiplies every trunk leaf by
1 - sum_t lr_t * wd_t (all three optimizers step on every update) and the target copy follows by the EMA on critic
steps only: the two trunks differ from the second step on.  oracle.drq_oracle's apply_gradients and target_update already restate
both; its critic_update however feeds the target critic the ONLINE trunk's next-frame features, and its update_high_utd computes
the features once at the head of the call.  This module holds

* the table of the wd_*.npz fixtures (the reference's own DrQAgent under oracle/jaxshim, recorded by the generator);
* a float64 restatement of critic_update, update_critics, update_high_utd and update that evaluates the target critic's encoder on
  features of the TARGET trunk (sac.py:143-147 with target_params) and recomputes the features before every optimizer step, built
  on O.encode, O.critic_forward, O.apply_gradients and O.target_update.
"""
import numpy as np
import torch
import torch.nn.functional as F

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


# ---- float64 restatement ---------------------------------------------------------------------------------------------------------
class _TargetTrunk:
    """what O.features reads of a TrainState, with the target copy of the trunk in the trunk's place"""

    def __init__(self, st):
        self.cfg, self.dtype, self.trunk = st.cfg, st.dtype, st.target_trunk


def features(st, frames, target=False):
    """{cam: u8 [N,H,W,3]} -> {cam: [N,h,w,512]} through the online trunk as it is NOW, or the target copy"""
    return O.features(_TargetTrunk(st) if target else st, frames)


def critic_update(st, feats_obs, feats_next, feats_next_target, state, next_state, action, reward, mask, noise, apply=True):
    """O.critic_update with the target critic's encoder on `feats_next_target`: forward_target_critic runs the whole network with
    target_params (sac.py:143-147), the trunk copy in them included; the policy at next_obs and the critic at obs keep the
    online trunk's features"""
    cfg = st.cfg
    with torch.no_grad():
        enc_pi = O.encode(st.params, cfg, feats_next, next_state, drop_masks=noise["mask_next"], stop_gradient=True)
        mean, std = O.policy_head(st.params, cfg, enc_pi)
        next_a, next_logp = O.sample_and_log_prob(mean, std, noise["eps_next"])
        enc_t = O.encode(st.target, cfg, feats_next_target, next_state)
        tq = O.critic_forward(st.target, cfg, enc_t, next_a)
        if cfg.subsample is None:
            min_q = tq.min(dim=0).values
        else:
            idx = [int(i) for i in np.asarray(noise["redq_idx"]).reshape(-1)[:cfg.subsample]]
            min_q = tq[idx].min(dim=0).values
        target_q = reward + cfg.discount * mask * min_q
        if cfg.backup_entropy:
            target_q = target_q - F.softplus(st.params["temp/lagrange"]).reshape(()) * next_logp
    p = {k: v.detach().clone().requires_grad_(True) for k, v in st.params.items()}
    enc = O.encode(p, cfg, feats_obs, state)
    q = O.critic_forward(p, cfg, enc, action)
    loss = ((q - target_q[None]) ** 2).mean()
    grads = O._grad_dict(loss, p)
    info = {"critic_loss": loss.item(), "predicted_qs": q.mean().item(), "target_qs": target_q.mean().item()}
    aux = {"target_q": target_q, "q": q.detach(), "grads": grads}
    if apply:
        O.apply_gradients(st, {"critic": grads})
        O.target_update(st)
    return info, aux


def _rows(d, lo, hi):
    return {k: v[lo:hi] for k, v in d.items()}


def _critic_rows(st, batch, noise, lo, hi, redq):
    """one critic step on rows [lo, hi) of the batch, from features of the trunks as they are now"""
    obs, nxt = _rows(batch["obs"], lo, hi), _rows(batch["next"], lo, hi)
    n = O._slice_noise(noise, lo, hi)
    if redq is not None:
        n["redq_idx"] = redq
    return critic_update(st, features(st, obs), features(st, nxt), features(st, nxt, target=True), batch["state"][lo:hi],
                         batch["next_state"][lo:hi], batch["action"][lo:hi], batch["reward"][lo:hi], batch["mask"][lo:hi], n)


def _redq(st, noise):
    return None if st.cfg.subsample is None else np.asarray(noise["redq_idx"]).reshape(-1, st.cfg.subsample)


def update_critics(st, batch, noise):
    """O.update_critics (drq.py:296-328) on both trunks"""
    redq = _redq(st, noise)
    return _critic_rows(st, batch, noise, 0, batch["reward"].shape[0], None if redq is None else redq[0])


def update_high_utd(st, batch, noise, utd_ratio=1):
    """O.update_high_utd (drq.py:255-294 -> sac.py:544-596): the reference applies after every critic minibatch, so minibatch i + 1
    sees the trunk after i + 1 decays and the actor step the trunk after all of them"""
    B = batch["reward"].shape[0]
    assert B % utd_ratio == 0, f"Batch size {B} must be divisible by UTD ratio {utd_ratio}"
    mb, redq, infos = B // utd_ratio, _redq(st, noise), []
    for i in range(utd_ratio):
        info, _ = _critic_rows(st, batch, noise, i * mb, (i + 1) * mb, None if redq is None else redq[i])
        infos.append(info)
    info = {k: float(np.mean([d[k] for d in infos])) for k in infos[0]}
    ainfo, aux = O.actor_temp_update(st, features(st, batch["obs"]), features(st, batch["next"]), batch["state"], batch["next_state"],
                                     noise)
    info.update(ainfo)
    return info, aux


def update(st, batch, noise, networks=("actor", "critic", "temperature")):
    """O.update (sac.py:243-299): every selected loss at the same parameters, one apply"""
    nets = set(networks)
    assert nets and nets <= {"actor", "critic", "temperature"}, f"Invalid gradient steps: {networks}"
    fo, fn = features(st, batch["obs"]), features(st, batch["next"])
    n = dict(noise)
    redq = _redq(st, noise) if "redq_idx" in noise else None
    if redq is not None:
        n["redq_idx"] = redq[0]
    info, grads = {}, {}
    if "critic" in nets:
        ci, caux = critic_update(st, fo, fn, features(st, batch["next"], target=True), batch["state"], batch["next_state"],
                                 batch["action"], batch["reward"], batch["mask"], n, apply=False)
        info.update(ci)
        grads["critic"] = caux["grads"]
    if nets & {"actor", "temperature"}:
        ai, aaux = O.actor_temp_update(st, fo, fn, batch["state"], batch["next_state"], n, apply=False, do_actor="actor" in nets,
                                       do_temp="temperature" in nets)
        info.update(ai)
        if "actor" in nets:
            grads["actor"] = aaux["g_actor"]
        if "temperature" in nets:
            grads["temperature"] = aaux["g_temp"]
    O.apply_gradients(st, grads)
    if "critic" in nets:
        O.target_update(st)
    return info


def run(cfg, steps, param_seed, module=None, dtype=torch.float64):
    """the recorded steps of a golden (oracle.golden_update.unpack) through the restatement -- or, with module=O, through the
    unmodified oracle (shared features) -> (TrainState, infos)"""
    from oracle import ref_update_runner as RR
    import sys
    m = module if module is not None else sys.modules[__name__]
    call = lambda name: getattr(m, name)  # noqa: E731
    trunk, theta = O.init_params(cfg, param_seed)
    st = O.TrainState(cfg, trunk, theta, dtype)
    infos = []
    for step in steps:
        b, n = RR.oracle_batch_and_noise(cfg, step, dtype)
        if step["kind"] == "critics":
            info, _ = call("update_critics")(st, b, n)
        elif step["kind"] == "high_utd":
            info, _ = call("update_high_utd")(st, b, n, step["utd"])
        else:
            info = call("update")(st, b, n, step["nets"])
        infos.append(info)
    return st, infos
