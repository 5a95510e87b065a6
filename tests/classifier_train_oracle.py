"""fp64 torch-autograd restatement of the reward classifier's train step (examples/async_cable_route_drq/
train_reward_classifier.py:122-137 over networks/reward_classifier.py:16-28), built on oracle/classifier_oracle.py and the
update oracle's primitives.  Pinned to tests/golden/classifier_train_*.npz (the reference's own modules under
oracle/jaxshim) by tests/test_classifier_train_cpu.py; the GPU tests use it for shapes the goldens do not hold.

Leaves are the product's flat names (trunk/..., enc/<image key>/..., head/...); only the camera heads and the classifier
head train.  Masks: {image key: bool [B, 4096], "head": bool [B, 256]} keep-masks of the two Dropout(0.1) layers."""
import numpy as np
import torch

from oracle import drq_oracle as O

KEEP = 0.9
CAM_LEAVES = ("sle", "dense/kernel", "dense/bias", "ln/scale", "ln/bias")
HEAD_LEAVES = ("head/dense0/kernel", "head/dense0/bias", "head/ln/scale", "head/ln/bias", "head/dense1/kernel", "head/dense1/bias")


def trainable(image_keys):
    return [f"enc/{k}/{leaf}" for k in image_keys for leaf in CAM_LEAVES] + list(HEAD_LEAVES)


def host_crop(frames, offsets, padding=4):
    """batched_random_crop (vision/data_augmentations.py:7-36): edge padding, then the (y, x) window of each frame.
    frames u8 [N, H, W, C], offsets int [N, 2]"""
    n, H, W, _ = frames.shape
    out = np.empty_like(frames)
    for i in range(n):
        p = np.pad(frames[i], ((padding, padding), (padding, padding), (0, 0)), mode="edge")
        y, x = int(offsets[i][0]), int(offsets[i][1])
        out[i] = p[y:y + H, x:x + W]
    return out


def features(params, image_keys, frames, dtype=torch.float64):
    """frames {k: u8 [B, H, W, 3]} -> {k: trunk features [B, h, w, 512] in `dtype`} (frozen: computed once per batch)"""
    tp = {k: torch.tensor(np.asarray(v), dtype=dtype) for k, v in params.items() if k.startswith("trunk/")}
    with torch.no_grad():
        return {k: O.trunk_forward(tp, torch.as_tensor(np.ascontiguousarray(frames[k])), dtype) for k in image_keys}


def hidden(th, image_keys, feats, masks=None):
    """reward_classifier.py:20-26, up to the ReLU; masks None = train=False (both Dropout layers are the identity)"""
    codes = []
    for k in image_keys:
        f = O.sle(feats[k], th[f"enc/{k}/sle"])                                   # resnet_v1.py:341-349
        if masks is not None:                                                     # :352 Dropout(0.1)
            f = torch.where(torch.as_tensor(masks[k]).bool(), f / KEEP, torch.zeros_like(f))
        z = f @ th[f"enc/{k}/dense/kernel"] + th[f"enc/{k}/dense/bias"]
        codes.append(torch.tanh(O.layer_norm(z, th[f"enc/{k}/ln/scale"], th[f"enc/{k}/ln/bias"])))
    x = torch.cat(codes, dim=-1)                                                  # encoding.py:51
    x = x @ th["head/dense0/kernel"] + th["head/dense0/bias"]                     # reward_classifier.py:23
    if masks is not None:                                                         # :24 Dropout before the LayerNorm
        x = torch.where(torch.as_tensor(masks["head"]).bool(), x / KEEP, torch.zeros_like(x))
    return torch.relu(O.layer_norm(x, th["head/ln/scale"], th["head/ln/bias"]))


def forward(th, image_keys, feats, masks=None):
    """reward_classifier.py:20-28"""
    return hidden(th, image_keys, feats, masks) @ th["head/dense1/kernel"] + th["head/dense1/bias"]


def sigmoid_bce(logits, labels):
    """optax.sigmoid_binary_cross_entropy: -labels log_sigmoid(l) - (1 - labels) log_sigmoid(-l)"""
    return -labels * torch.nn.functional.logsigmoid(logits) - (1.0 - labels) * torch.nn.functional.logsigmoid(-logits)


class State:
    """params / mu / nu as fp64 numpy flat dicts (moments of the trainable leaves only), step.  dtype: the precision train_step
    computes the forward, the loss and the gradients in (float32 = the yardstick of what plain fp32 attains)"""

    def __init__(self, params, image_keys, lr=1e-4, dtype=torch.float64):
        self.keys, self.dtype = tuple(image_keys), dtype
        self.params = {k: np.asarray(v, np.float64).copy() for k, v in params.items()}
        self.mu = {k: np.zeros_like(self.params[k]) for k in trainable(self.keys)}
        self.nu = {k: np.zeros_like(self.params[k]) for k in trainable(self.keys)}
        self.shapes = {k: np.shape(v) for k, v in params.items()}
        self.step, self.lr = 0, lr


def train_step(st: State, feats, labels, masks):
    """One train_step: -> (loss, accuracy, eval logits, grads); st is updated (optax.adam(lr), b1 0.9, b2 0.999, eps 1e-8)"""
    th = {k: torch.tensor(st.params[k].reshape(st.shapes[k]), dtype=st.dtype, requires_grad=True) for k in trainable(st.keys)}
    y = torch.as_tensor(np.asarray(labels, np.float64).reshape(-1, 1)).to(st.dtype)
    logits = forward(th, st.keys, feats, masks)
    loss = sigmoid_bce(logits, y).mean()
    grads = torch.autograd.grad(loss, [th[k] for k in trainable(st.keys)])
    with torch.no_grad():
        ev = forward(th, st.keys, feats, None)
        acc = ((torch.sigmoid(ev) >= 0.5).to(st.dtype) == y).double().mean()
    st.step += 1
    t = st.step
    g_out = {}
    for k, g in zip(trainable(st.keys), grads):
        g = g.detach().double().numpy().reshape(-1)
        g_out[k] = g
        st.mu[k] = 0.9 * st.mu[k].reshape(-1) + 0.1 * g
        st.nu[k] = 0.999 * st.nu[k].reshape(-1) + 0.001 * g * g
        mh = st.mu[k] / (1.0 - 0.9 ** t)
        nh = st.nu[k] / (1.0 - 0.999 ** t)
        st.params[k] = st.params[k].reshape(-1) - st.lr * mh / (np.sqrt(nh) + 1e-8)
    return float(loss.detach()), float(acc), ev.detach().double().numpy(), g_out
