"""Torch-autograd restatement of the whole behaviour-cloning update (serl_launcher/agents/continuous/bc.py:37-116 over
networks/actor_critic_nets.py:167-227, networks/mlp.py and common/encoding.py:26-72), built on the update oracle's primitives
beside tests/classifier_train_oracle.py.  tests/test_bc_cpu.py::_np_bc restates the head and the MLP only, from a recorded
encoder output; this one starts at the frames: frozen trunk, camera heads with injected Dropout keep-masks (behind
stop_gradient), the trainable proprio Dense -> LayerNorm -> tanh, Dense -> tanh twice WITHOUT LayerNorm, the mean / log-std heads,
std = clip(exp(log_std), std_min, std_max), actor_loss = -mean_b sum_a log N(a | mean, std), mse, the gradients of the twelve
trainable leaves by autograd, sample_actions, get_debug_metrics, and one optax.adam step.  Pinned to tests/golden/bc_*.npz (the
reference's own BCAgent under oracle/jaxshim) and to _np_bc by tests/test_learner_regimes_cpu.py.

`dtype` switches every tensor (trunk included) between float64 -- the reference of the GPU tests -- and float32: the yardstick
that says what a plain fp32 implementation attains."""
import math

import numpy as np
import torch

from oracle import drq_oracle as O

TRAIN = ("enc/proprio/dense/kernel", "enc/proprio/dense/bias", "enc/proprio/ln/scale", "enc/proprio/ln/bias",
         "actor/w1", "actor/b1", "actor/w2", "actor/b2", "actor/mean/kernel", "actor/mean/bias",
         "actor/logstd/kernel", "actor/logstd/bias")
HEAD_LEAVES = ("actor/mean/kernel", "actor/mean/bias", "actor/logstd/kernel", "actor/logstd/bias")


def bc_theta(theta):
    """the BC leaves of an O.init_params theta (camera heads, proprio branch, MLP without its LayerNorms, the two heads)"""
    return {k: v for k, v in theta.items() if k in TRAIN or (k.startswith("enc/") and not k.startswith("enc/proprio"))}


def features(trunk, cfg, frames, dtype=torch.float64):
    """frames {k: u8 [B, H, W, 3]} -> {k: trunk features [B, h, w, 512]} (frozen: once per batch)"""
    tp = O.to_torch(trunk, dtype)
    with torch.no_grad():
        return {k: O.trunk_forward(tp, torch.as_tensor(np.ascontiguousarray(frames[k])), dtype) for k in cfg.image_keys}


def policy(th, cfg, feats, state, masks=None):
    """Policy.__call__ up to the distribution's parameters -> (mean, log_std, std at temperature 1, (enc, h1, h2))"""
    enc = O.encode(th, cfg, feats, state, drop_masks=masks, stop_gradient=True)        # actor_critic_nets.py:179-187
    h1 = torch.tanh(enc @ th["actor/w1"] + th["actor/b1"])                              # mlp.py:26-34, use_layer_norm=False
    h2 = torch.tanh(h1 @ th["actor/w2"] + th["actor/b2"])
    mean = h2 @ th["actor/mean/kernel"] + th["actor/mean/bias"]
    log_std = h2 @ th["actor/logstd/kernel"] + th["actor/logstd/bias"]
    std = torch.clamp(torch.exp(log_std), cfg.std_min, cfg.std_max)                     # :205-210 (then * sqrt(temperature))
    return mean, log_std, std, (enc, h1, h2)


def log_prob(mean, std, action):
    """distrax.MultivariateNormalDiag.log_prob"""
    z = (action - mean) / std
    return (-0.5 * z * z - torch.log(std) - 0.5 * math.log(2.0 * math.pi)).sum(-1)


class State:
    """params (every leaf, numpy in `dtype`'s precision), Adam moments of the trainable leaves, step"""

    def __init__(self, cfg, trunk, theta, dtype=torch.float64, lr=3e-4):
        self.cfg, self.dtype, self.lr, self.step = cfg, dtype, lr, 0
        self.trunk = trunk
        self.params = O.to_torch(bc_theta(theta), dtype)
        self.mu = {k: torch.zeros_like(self.params[k]) for k in TRAIN}
        self.nu = {k: torch.zeros_like(self.params[k]) for k in TRAIN}

    def tensor(self, a):
        return torch.as_tensor(np.asarray(a)).to(self.dtype)

    def masks(self, masks):
        return None if masks is None else {k: torch.as_tensor(np.asarray(m)) for k, m in masks.items()}


def update(st: State, feats, state, action, masks):
    """BCAgent.update -> (info {actor_loss, mse}, {leaf: gradient}, aux {mean, log_std, h1, h2}); st takes one optax.adam(lr) step
    (b1 0.9, b2 0.999, eps 1e-8, no schedule: bc.py:139)"""
    th = {k: (v.clone().requires_grad_(True) if k in TRAIN else v) for k, v in st.params.items()}
    a = st.tensor(action)
    mean, log_std, std, (enc, h1, h2) = policy(th, st.cfg, feats, st.tensor(state), st.masks(masks))
    loss = -log_prob(mean, std, a).mean()
    mse = ((mean - a) ** 2).sum(-1).mean()
    grads = dict(zip(TRAIN, torch.autograd.grad(loss, [th[k] for k in TRAIN])))
    st.step += 1
    t = st.step
    for k, g in grads.items():
        st.mu[k] = 0.9 * st.mu[k] + 0.1 * g
        st.nu[k] = 0.999 * st.nu[k] + 0.001 * g * g
        mh, nh = st.mu[k] / (1.0 - 0.9 ** t), st.nu[k] / (1.0 - 0.999 ** t)
        st.params[k] = st.params[k] - st.lr * mh / (torch.sqrt(nh) + 1e-8)
    aux = {"mean": mean.detach(), "log_std": log_std.detach(), "h1": h1.detach(), "h2": h2.detach(), "enc": enc.detach()}
    return {"actor_loss": float(loss.detach()), "mse": float(mse.detach())}, grads, aux


def sample_actions(st: State, feats, state, eps=None, temperature=1.0):
    """BCAgent.sample_actions (train=False): eps None = argmax (the mode: the mean, no tanh), else mean + std sqrt(T) eps"""
    with torch.no_grad():
        mean, _, std, _ = policy(st.params, st.cfg, feats, st.tensor(state))
        return mean if eps is None else mean + std * math.sqrt(temperature) * st.tensor(eps)


def debug_metrics(st: State, feats, state, action):
    """BCAgent.get_debug_metrics (train=False, temperature 1) -> {mse [B], log_probs [B], pi_actions [B, A]}"""
    with torch.no_grad():
        a = st.tensor(action)
        mean, _, std, _ = policy(st.params, st.cfg, feats, st.tensor(state))
        return {"mse": ((mean - a) ** 2).sum(-1), "log_probs": log_prob(mean, std, a), "pi_actions": mean}
