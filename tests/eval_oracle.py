"""Shared by tests/test_evaluate_cpu.py, tests/test_evaluate_gpu.py and tests/golden/make_golden_eval.py: a restatement, in the
dtype of the caller's choice, of the four read-only questions a learner answers without a step --

  q, q_target   forward_critic(obs, actions, train=False) with params / with target_params      (sac.py:33-69)
  mean, std     forward_policy(obs, train=False).distribution.loc / .scale_diag                  (sac.py:71-91)
  mode          .mode(): tanh(loc), or loc without the squash
  log_prob      .log_prob(actions): distrax Transformed.log_prob under the Tanh bijector, u = atanh(a),
                sum_j [log N(u_j; loc_j, scale_j) - 2 (log 2 - u_j - softplus(-2 u_j))]; the diagonal Gaussian's without the squash

-- from oracle.drq_oracle (encode, critic_forward, policy_head; the distribution is the Config's), and the table of the eval_*.npz fixtures with the
parameters and inputs each was recorded from.  atanh is formed as (log1p(a) - log1p(-a)) / 2, as the kernel forms it; a row with
an action component of exactly +-1 is not finite, here, in the kernel and in the reference."""
import dataclasses
import math

import numpy as np
import torch

from oracle import drq_oracle as O
import golden_replay as GR
import policy_modes as PM
import trained_regime as TR

QUANTITIES = ("q", "q_target", "mean", "std", "mode", "log_prob")
ACTION_BOUND = 1.0 - 2.0 ** -10       # stored actions of the fixtures: exact fp32 inputs with a well-conditioned atanh
BATCH_SEED = 31

# name -> (oracle Config, rows, (std_parameterization, tanh_squash_distribution): what the Config holds, for the check against a
# file's meta).  The files are eval_<name>.npz: no update_*.npz / init_*.npz glob picks them up.
_STATE = dict(image_keys=(), S=10, A=4, discount=0.99, temp_warmup=0, warmup=4)
GOLDEN = {
    "sac_state": (O.Config(**_STATE), 8, ("exp", True)),
    "drq_one_cam": (O.Config(image_keys=("image",), H=64, W=64, S=5, A=3), 6, ("exp", True)),
    "sac_state_softplus_gauss": (PM.mode_config("softplus", False, **_STATE), 8, ("softplus", False)),
    "sac_state_uniform": (PM.mode_config("uniform", True, **_STATE), 8, ("uniform", True)),
}


def golden_path(name):
    return GR.variant_path("eval", name)


def mode_theta(theta, cfg):
    """O.init_params' leaves of the launcher's ("exp") policy -> the trained-regime leaves of a case (tests/trained_regime.trained_like; "uniform": the log-std Dense
    gives way to actor/log_stds = its bias cycle)"""
    out = TR.trained_like(theta, cfg, lam=0.5)
    if cfg.std_parameterization == "uniform":
        out["actor/log_stds"] = out["actor/logstd/bias"].copy()
        for k in PM.STD_DENSE:
            del out[k]
    return out


def leaves(cfg, param_seed=GR.PARAM_SEED):
    """-> (trunk, online theta, target theta): trained-regime leaves and a target copy that differs (perturb_target)"""
    trunk, theta = O.init_params(dataclasses.replace(cfg, std_parameterization="exp"), param_seed)
    theta = mode_theta(theta, cfg)
    return trunk, theta, TR.perturb_target(theta, cfg)


def scaled_actions(a):
    """stored actions with max |a| <= 1 - 2^-10, float32"""
    return (np.asarray(a, np.float32) * np.float32(ACTION_BOUND)).astype(np.float32)


def golden_inputs(name):
    """-> the reference-format sample a fixture was recorded on (oracle.ref_update_runner.synth_*_batch, actions scaled)"""
    from oracle import ref_update_runner as RR
    cfg, B, _ = GOLDEN[name]
    pb = RR.synth_flat_batch(cfg, B, BATCH_SEED) if cfg.state_only else RR.synth_packed_batch(cfg, B, BATCH_SEED)
    pb["action"] = scaled_actions(pb["action"])
    return pb


def log_prob(mean, sd, a, squash):
    """log pi(a | s) [rows] in the dtype of the arguments"""
    if squash:
        u = 0.5 * (torch.log1p(a) - torch.log1p(-a))
    else:
        u = a
    z = (u - mean) / sd
    lp = (-0.5 * z * z - torch.log(sd) - 0.5 * math.log(2.0 * math.pi)).sum(-1)
    if not squash:
        return lp
    return lp - (2.0 * (math.log(2.0) - u - torch.nn.functional.softplus(-2.0 * u))).sum(-1)


def evaluate(cfg, trunk, theta, target, frames, state, actions, dtype=torch.float64):
    """frames {camera: u8[n, H, W, 3]} (numpy; {} state-only), state f32[n, S], actions f32[n, A] -> {quantity: numpy array} in
    `dtype` arithmetic: q, q_target [ensemble, n]; mean, std, mode [n, A]; log_prob [n]; the policy distribution is cfg's"""
    st = O.TrainState(cfg, trunk, theta, dtype)
    tgt = O.to_torch(target, dtype)
    s, a = torch.tensor(np.asarray(state), dtype=dtype), torch.tensor(np.asarray(actions), dtype=dtype)
    with torch.no_grad():
        feats = O.features(st, {k: torch.as_tensor(np.asarray(v)) for k, v in frames.items()})
        enc = O.encode(st.params, cfg, feats, s)
        enc_t = O.encode(tgt, cfg, feats, s)
        mean, sd = O.policy_head(st.params, cfg, enc)
        squash = cfg.tanh_squash
        out = {"q": O.critic_forward(st.params, cfg, enc, a), "q_target": O.critic_forward(tgt, cfg, enc_t, a),
               "mean": mean, "std": sd, "mode": torch.tanh(mean) if squash else mean, "log_prob": log_prob(mean, sd, a, squash)}
    return {k: v.detach().cpu().numpy() for k, v in out.items()}


def row_error(got, ref):
    """log_prob's measure: per row |got - ref| / max(1, |ref|), the worst row (one large row cannot hide a small one)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))))


def log_prob_yardstick(cfg, trunk, theta, target, frames, state, actions):
    """-> (fp64 results, error of the fp32 restatement's log_prob against them under row_error)"""
    r64 = evaluate(cfg, trunk, theta, target, frames, state, actions, torch.float64)
    r32 = evaluate(cfg, trunk, theta, target, frames, state, actions, torch.float32)
    return r64, row_error(r32["log_prob"], r64["log_prob"])
