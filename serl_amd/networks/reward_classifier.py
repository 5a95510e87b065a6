"""Reward classifier with the reference's names (serl_launcher/networks/reward_classifier.py and
examples/async_cable_route_drq/train_reward_classifier.py):

    create_classifier(key, sample, image_keys, pretrained_encoder_path)   (:31-90)
    load_classifier_func(key, sample, image_keys, checkpoint_path, step)  (:93-113) -> func(obs) -> logits
    train_step(state, batch, key) -> (state, loss, train_accuracy)       (train_reward_classifier.py:122-137)
    train_reward_classifier(pos_buffer, neg_buffer, image_keys, ...)     (train_reward_classifier.py:54-172)

The forward pass (frozen ResNet-10 trunk -> per camera SpatialLearnedEmbeddings / Dropout / Dense / LayerNorm / tanh ->
Dense(256) -> Dropout -> LayerNorm -> ReLU -> Dense(1)) and, for a classifier created with trainable=True, the train step
(loss, backward, optax.adam) run in libserl_mi355.so (csrc/classifier.hip); no CPU fallback.  Checkpoints use the flax
msgpack layout of the reference's TrainState (utils/checkpoint.py).
"""
from __future__ import annotations

import ctypes as C
import os
import pickle
from typing import Callable, Dict, List, Optional

import numpy as np
import torch

from .. import _lib
from .. import jaxrng as J
from .._handle import Handle
from .._lib_agent import SerlClassifierCfg
from ..agents.flax_tree import CAM_PATHS as _CAM_PATHS
from ..agents.flax_tree import (AdamTrainState, _camera_shapes, _trunk_paths, leaves_from_tree, tree_from_leaves,
                                trunk_from_flax, trunk_owner)
from ..agents.flax_tree import EmptyState, ScaleByAdamState  # noqa: F401  (the types `opt_state` holds, importable from here)
from ..utils.init import trunk_shapes


_HEAD_PATHS = {   # flat leaf -> path in BinaryClassifier's parameter tree (flax auto-names, reward_classifier.py:20-28)
    "head/dense0/kernel": ("Dense_0", "kernel"), "head/dense0/bias": ("Dense_0", "bias"),
    "head/ln/scale": ("LayerNorm_0", "scale"), "head/ln/bias": ("LayerNorm_0", "bias"),
    "head/dense1/kernel": ("Dense_1", "kernel"), "head/dense1/bias": ("Dense_1", "bias"),
}

SLE_DIM = 512 * 8
HIDDEN = 256


def _tree_paths(image_keys):
    """flat leaf -> path in the parameter tree: the camera heads under encoder_def/encoder_<key>, the ONE shared frozen
    trunk under the first camera in sorted-key order (:37-51), the classifier head at the root."""
    m = {}
    for i, k in enumerate(image_keys):
        for leaf, sub in _CAM_PATHS.items():
            m[f"enc/{i}/{leaf}"] = ("encoder_def", f"encoder_{k}") + sub
    for leaf, sub in _trunk_paths().items():
        m[leaf] = ("encoder_def", f"encoder_{trunk_owner(image_keys)}", "pretrained_encoder") + sub
    return {**m, **_HEAD_PATHS}


def _tree_shapes(image_keys, H, W):
    """flat leaf -> flax shape"""
    sh = dict(trunk_shapes(), **_camera_shapes(len(image_keys), H, W, 256))
    sh["head/dense0/kernel"], sh["head/dense0/bias"] = (256 * len(image_keys), HIDDEN), (HIDDEN,)
    sh["head/ln/scale"] = sh["head/ln/bias"] = (HIDDEN,)
    sh["head/dense1/kernel"], sh["head/dense1/bias"] = (HIDDEN, 1), (1,)
    return sh


def dropout_paths(image_keys) -> List[tuple]:
    """Scope paths of the classifier's Dropout layers: encoder_def/encoder_<k>/Dropout_0 behind every camera's
    SpatialLearnedEmbeddings (resnet_v1.py:352, shape (B, 4096)), then the root Dropout_0 (reward_classifier.py:24, (B, 256))."""
    return [("encoder_def", f"encoder_{k}", "Dropout_0") for k in image_keys] + [("Dropout_0",)]


def dropout_keys(key, image_keys) -> np.ndarray:
    """uint32[n_cam + 1][2]: the keys make_rng("dropout") gives those layers under apply_fn(..., rngs={"dropout": key})"""
    k = np.asarray(key, np.uint32).reshape(2)
    return np.stack([J.flax_make_rng(k, p) for p in dropout_paths(image_keys)]).astype(np.uint32)


def _stacked(frames):
    """torch.stack(frames) -- without the copy when the cameras already lie back to back in one contiguous buffer
    (train_reward_classifier's batches: views of one [n_cam][B][H][W][3] tensor)"""
    f0 = frames[0]
    step = f0.numel()
    if all(f.is_contiguous() and f.shape == f0.shape and f.untyped_storage().data_ptr() == f0.untyped_storage().data_ptr()
           and f.storage_offset() == f0.storage_offset() + i * step for i, f in enumerate(frames)):
        return f0.as_strided((len(frames),) + tuple(f0.shape), (step,) + tuple(f0.stride()), f0.storage_offset())
    return torch.stack(frames).contiguous()


class Classifier(Handle, AdamTrainState):
    """The role of the reference's `TrainState`: `.params` (flax-layout tree) and
    `.apply_fn({"params": params}, obs, train=False)`; parameters live in HBM.  With trainable=True also `.step`,
    `.opt_state` (optax.adam's (ScaleByAdamState(count, mu, nu), EmptyState()); the frozen trunk's moments are zeros),
    apply_fn(..., train=True, rngs={"dropout": key}) and `train_step`."""

    prefix = "serl_classifier"
    opt_state = property(AdamTrainState.adam_state)

    def __init__(self, image_keys, H, W, max_batch=64, device=0, trainable=False, learning_rate=1e-4):
        self.image_keys = tuple(image_keys)
        self.H, self.W, self.max_batch, self.device = H, W, max_batch, device
        super().__init__(SerlClassifierCfg(device, len(self.image_keys), H, W, max_batch))
        self.trainable = bool(trainable)
        if self.trainable:   # TrainState.create(tx=optax.adam(learning_rate)) (reward_classifier.py:62-66)
            _lib.check(self.L.serl_classifier_train_init(self._h, int(max_batch), float(learning_rate), 0.9, 0.999, 1e-8))

    # ---- flat leaves: the public set / get address the parameters, _set / _get any section ("params", "opt/mu", "opt/nu")
    _set, _get = Handle.set, Handle.get

    def set(self, leaf, value):
        self._set("params", leaf, value)

    def get(self, leaf):
        return self._get("params", leaf)

    def _leaf_call(self, op, section, leaf, data, count):
        if section != "params":   # the Adam moments of the training state
            return super()._leaf_call("train_" + op, section, leaf, data, count)
        if op == "set":
            self._params_cache = None
        return self._fn(op)(self._h, leaf.encode(), data, count)

    def _leaf(self, k, leaf):
        return f"enc/{self.image_keys.index(k)}/{leaf}"

    def load_flat(self, flat: Dict[str, np.ndarray]):
        """flat: trunk leaves, 'enc/<image key>/...', 'head/...'."""
        for name, v in flat.items():
            if name.startswith("enc/"):
                _, k, leaf = name.split("/", 2)
                name = self._leaf(k, leaf)
            self.set(name, v)
        return self

    # ---- flax layout (reward_classifier.py:58-60: classifier_def.init(key, sample)["params"])
    @property
    def params(self):
        """The flax-layout tree (built from HBM once, cached until a leaf is set)."""
        if self._params_cache is None:
            self._params_cache = self._export()
        return self._params_cache

    def _export(self, section="params"):
        return tree_from_leaves(_tree_paths(self.image_keys), _tree_shapes(self.image_keys, self.H, self.W),
                                lambda leaf: self._get(section, leaf))

    def load_params(self, tree, section="params"):
        """A BinaryClassifier parameter tree (e.g. the `params` entry of a checkpoint the reference's trainer wrote); with
        section "opt/mu" / "opt/nu" an Adam moment tree of the same layout."""
        trunk = _trunk_paths()
        heads = {leaf: p for leaf, p in _tree_paths(self.image_keys).items() if leaf not in trunk}
        for leaf, v in leaves_from_tree(heads, tree):
            self._set(section, leaf, v)
        for k in self.image_keys:   # the shared trunk, under whichever camera holds it
            sub = tree["encoder_def"][f"encoder_{k}"]
            if "pretrained_encoder" in sub:
                for leaf, v in trunk_from_flax(sub["pretrained_encoder"]).items():
                    self._set(section, leaf, v)
        return self

    _import = load_params

    def replace(self, params=None, **kw):
        """flax TrainState.replace; an inference-only classifier takes `params` only."""
        if not kw:
            return self if params is None else self.load_params(params)
        self._need_training()
        return super().replace(params=params, **kw)

    # ---- training state (flax TrainState fields, reward_classifier.py:61-66)
    def _need_training(self):
        if not self.trainable:
            raise NotImplementedError("classifier training needs create_classifier(..., trainable=True)")

    @property
    def step(self) -> int:
        self._need_training()
        out = C.c_int64()
        _lib.check(self.L.serl_classifier_train_get_step(self._h, C.byref(out)))
        return int(out.value)

    def _set_step(self, step):
        _lib.check(self.L.serl_classifier_train_set_step(self._h, step))

    def load_state_dict(self, sd: dict):
        self._need_training()
        return super().load_state_dict(sd)

    def _device_frames(self, observations):
        """{image_key: u8 (T=1, H, W, 3) or (B, T=1, H, W, 3), host or device} -> (u8[n_cam][n][H][W][3] on the device, batched)"""
        dev = torch.device("cuda", self.device)
        frames, batched = [], None
        for k in self.image_keys:
            x = torch.as_tensor(observations[k])
            if x.dtype != torch.uint8:
                raise TypeError(f"observation '{k}' must be uint8 (got {x.dtype})")
            batched = x.dim() == 5 if batched is None else batched
            x = x if batched else x[None]
            if x.shape[1] != 1:
                raise NotImplementedError("frame stacking T > 1 is not supported")
            frames.append(x[:, 0].to(dev))
        return _stacked(frames), batched

    def _dropout_args(self, n, key, masks, dev):
        """(device keep-mask buffer or None, host keys) of the two Dropout layers.  masks: optional injected keep-masks
        {image key: u8[n, 4096], "head": u8[n, 256]} (parity tests); by default they are drawn from `key` in the kernels."""
        keys = np.ascontiguousarray(dropout_keys(np.zeros(2, np.uint32) if key is None else key, self.image_keys).reshape(-1))
        if masks is None:
            if key is None:
                raise ValueError("train=True needs rngs={'dropout': key} or injected masks")
            return None, keys
        parts = [torch.as_tensor(np.asarray(masks[k], np.uint8)).reshape(-1) for k in self.image_keys]
        parts.append(torch.as_tensor(np.asarray(masks["head"], np.uint8)).reshape(-1))
        buf = torch.cat(parts).to(dev).contiguous()
        if buf.numel() != n * (len(self.image_keys) * SLE_DIM + HIDDEN):
            raise ValueError("injected Dropout masks must be u8[n, 4096] per camera and u8[n, 256] for 'head'")
        return buf, keys

    def train_logits(self, observations, key=None, masks=None) -> np.ndarray:
        """apply_fn(..., train=True, rngs={"dropout": key}): logits with both Dropout layers active, no update -> (B, 1)"""
        self._need_training()
        fr, batched = self._device_frames(observations)
        n = fr.shape[1]
        mbuf, keys = self._dropout_args(n, key, masks, fr.device)
        out = torch.empty((n,), dtype=torch.float32, device=fr.device)
        _lib.check(self.L.serl_classifier_train_forward(self._h, C.c_void_p(fr.data_ptr()), n,
                                                        None if mbuf is None else C.c_void_p(mbuf.data_ptr()),
                                                        keys.ctypes.data_as(C.c_void_p), C.c_void_p(out.data_ptr()), self._stream()))
        o = out.cpu().numpy().reshape(n, 1)
        return o if batched else o[0]

    def train_step(self, batch, key, masks=None):
        """train_reward_classifier.py:122-137 on this classifier: batch = {"data": observations (B, 1, H, W, 3) u8 (host or
        device), "labels": (B, 1)}.  Returns (self, loss, train_accuracy) -- 0-d device tensors, read when used."""
        self._need_training()
        fr, _ = self._device_frames(batch["data"])
        n = fr.shape[1]
        lab = batch["labels"]
        lab = torch.as_tensor(lab if torch.is_tensor(lab) else np.asarray(lab, np.float32), dtype=torch.float32)
        lab = lab.reshape(-1).to(fr.device).contiguous()
        if lab.numel() != n:
            raise ValueError(f"labels hold {lab.numel()} values for {n} observations")
        mbuf, keys = self._dropout_args(n, key, masks, fr.device)
        s = self._stream()
        _lib.check(self.L.serl_classifier_train_step(self._h, C.c_void_p(fr.data_ptr()), n, C.c_void_p(lab.data_ptr()),
                                                     None if mbuf is None else C.c_void_p(mbuf.data_ptr()),
                                                     keys.ctypes.data_as(C.c_void_p), s))
        info = torch.empty(2, dtype=torch.float32, device=fr.device)
        _lib.check(self.L.serl_classifier_read_train_info(self._h, C.c_void_p(info.data_ptr()), s))
        self._params_cache = None
        self._inflight = (fr, lab, mbuf)   # (alive until the stream has consumed them)
        return self, info[0], info[1]

    # ---- forward
    def logits(self, observations) -> np.ndarray:
        """observations: {image_key: u8 (T=1, H, W, 3) or (B, T=1, H, W, 3)} (encoding.py:39-44 stacking) -> (1,) / (B, 1)."""
        first = np.asarray(observations[self.image_keys[0]])
        batched = first.ndim == 5
        frames = []
        for k in self.image_keys:
            x = np.asarray(observations[k])
            if x.dtype != np.uint8:
                raise TypeError(f"observation '{k}' must be uint8 (got {x.dtype})")
            x = x if batched else x[None]
            if x.shape[1] != 1:
                raise NotImplementedError("frame stacking T > 1 is not supported")
            frames.append(x[:, 0])
        fr = np.stack(frames)                                  # [n_cam][n][H][W][3]
        n = fr.shape[1]
        out = np.empty((n, 1), np.float32)
        dev = torch.device("cuda", self.device)
        for lo in range(0, n, self.max_batch):
            hi = min(n, lo + self.max_batch)
            d_fr = torch.from_numpy(np.ascontiguousarray(fr[:, lo:hi])).to(dev)
            d_out = torch.empty((hi - lo,), dtype=torch.float32, device=dev)
            st = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(self.L.serl_classifier_logits(self._h, d_fr.data_ptr(), hi - lo, d_out.data_ptr(), C.c_void_p(st)))
            out[lo:hi, 0] = d_out.cpu().numpy()
        return out if batched else out[0]

    def apply_fn(self, variables, observations, train=False, rngs=None, masks=None, **kw):
        if train and not self.trainable:
            raise NotImplementedError("classifier training needs create_classifier(..., trainable=True)")
        p = None if variables is None else variables.get("params")
        if p is not None and p is not self._params_cache:    # foreign parameters: load them first
            self.load_params(p)
        if train:
            return self.train_logits(observations, None if rngs is None else rngs.get("dropout"), masks)
        return self.logits(observations)

    _params_cache = None


def create_classifier(key, sample: Dict, image_keys: List[str], pretrained_encoder_path: str = "./resnet10_params.pkl",
                      max_batch: int = 64, device: int = 0, trainable: bool = False, learning_rate: float = 1e-4,
                      param_init: str = "numpy") -> Classifier:
    """reward_classifier.py:31-90: a freshly initialised classifier whose frozen trunk holds the pretrained ResNet-10.
    trainable=True adds optax.adam(learning_rate)'s state and the train step for batches of up to max_batch rows.
    param_init: "numpy" (default) or "reference" (classifier_def.init(key, sample)'s keys and initialisers, utils/init_ref.py)."""
    from ..utils import init as pinit
    from ..utils import init_ref
    reference = init_ref.check_param_init(param_init)
    first = np.asarray(sample[image_keys[0]])
    H, W = int(first.shape[-3]), int(first.shape[-2])
    seed = int(np.asarray(key).reshape(-1)[-1]) if not isinstance(key, int) else key
    c = Classifier(image_keys, H, W, max_batch=max_batch, device=device, trainable=trainable, learning_rate=learning_rate)
    theta = init_ref.classifier_reference(image_keys, H, W, key, device=device) if reference else \
        pinit.init_classifier(len(image_keys), H, W, seed)
    for name, v in theta.items():
        c.set(name, v)
    with open(pretrained_encoder_path, "rb") as f:
        encoder_params = pickle.load(f)
    for leaf, v in trunk_from_flax(encoder_params).items():   # top-level keys the pickle lacks keep their value (:76-86)
        c.set(leaf, v)
    return c


def load_classifier_func(key, sample: Dict, image_keys: List[str], checkpoint_path: str, step: Optional[int] = None,
                         pretrained_encoder_path: str = "./resnet10_params.pkl") -> Callable[[Dict], np.ndarray]:
    """reward_classifier.py:93-113: restore `checkpoint_path` (a directory of checkpoint_<step> files or one file, flax
    msgpack layout of the classifier TrainState) and return obs -> logits."""
    from ..utils.checkpoint import read_checkpoint_tree
    classifier = create_classifier(key, sample, image_keys, pretrained_encoder_path) if os.path.exists(pretrained_encoder_path) \
        else _blank_classifier(sample, image_keys)
    tree = read_checkpoint_tree(checkpoint_path, step)
    classifier.load_params(tree["params"])
    return lambda obs: classifier.logits(obs)


def _blank_classifier(sample, image_keys):
    first = np.asarray(sample[image_keys[0]])
    return Classifier(image_keys, int(first.shape[-3]), int(first.shape[-2]))


def train_step(state: Classifier, batch: Dict, key, masks=None):
    """train_reward_classifier.py:122-137 (the jitted train_step): loss = mean(optax.sigmoid_binary_cross_entropy(
    apply_fn(params, data, rngs={"dropout": key}, train=True), labels)), one optax.adam step, and train_accuracy =
    mean((sigmoid(apply_fn(params, data, train=False)) >= 0.5) == labels) with the pre-update parameters.
    Returns (state, loss, train_accuracy); state is updated in place."""
    return state.train_step(batch, key, masks=masks)


def _demo_sample(store, image_keys):
    H, W, _ = store._img_shape
    return {k: np.zeros((1, 1, H, W, 3), np.uint8) for k in image_keys}


def train_reward_classifier(pos_buffer, neg_buffer, image_keys: List[str], *, batch_size: int = 256, num_epochs: int = 100,
                            classifier_ckpt_path: Optional[str] = None, pretrained_encoder_path: str = "./resnet10_params.pkl",
                            init_params: Optional[Dict[str, np.ndarray]] = None, device: int = 0, verbose: bool = True):
    """The loop of train_reward_classifier.py:54-172 on the HBM data stores (MemoryEfficientReplayBufferDataStore filled with
    positive / negative demos):
      rng = PRNGKey(0); rng, _ = split(rng); one shape-only draw from each store (:101-105); rng, key = split(rng);
      create_classifier(key, ...); per epoch: B/2 indices from each store, sample = concat(pos next_observations,
      neg observations), rng, key = split(rng) -> batched_random_crop(sample, key, padding=4) (one key: every camera shifts
      sample i by the same offset), labels [1]*B/2 + [0]*B/2, rng, key = split(rng) -> train_step;
      at the end checkpoints.save_checkpoint(classifier_ckpt_path, classifier, step=num_epochs, overwrite=True).
    The frames go from the stores to the trunk without leaving HBM (serl_rb_gather_crop does the gather and the crop).
    init_params: optional flat leaves loaded over the fresh classifier (parity tests inject parameters).
    Returns (classifier, log) with log = {"loss", "accuracy", "pos_idx", "neg_idx", "crop"} per epoch."""
    from ..agents.batch import DeviceBatch
    from ..data.data_store import gather_crop
    image_keys = list(image_keys)
    half = batch_size // 2
    rng = J.prngkey(0)
    rng, _ = J.split(rng)
    pos_buffer.sample_indices(half)   # next(pos_iterator) / next(neg_iterator): shapes only, but they advance np_random
    neg_buffer.sample_indices(half)
    rng, key = J.split(rng)
    classifier = create_classifier(key, _demo_sample(pos_buffer, image_keys), image_keys, pretrained_encoder_path,
                                   max_batch=batch_size, device=device, trainable=True)
    if init_params is not None:
        classifier.load_flat(init_params)
    H, W, Cc = pos_buffer._img_shape
    dbs = [DeviceBatch(half, len(image_keys), H, W, Cc, s._S, s._A, device) for s in (pos_buffer, neg_buffer)]
    labels = torch.cat([torch.ones(half), torch.zeros(half)]).to(torch.device("cuda", device))
    log = {"loss": [], "accuracy": [], "pos_idx": [], "neg_idx": [], "crop": []}
    pending = []
    for epoch in range(num_epochs):
        ip, ineg = pos_buffer.sample_indices(half), neg_buffer.sample_indices(half)
        rng, key = J.split(rng)
        crop = J.crop_offsets(key, 2 * half, padding=4)
        gather_crop([(pos_buffer, ip)], None, crop[:half], dbs[0])     # positives: next_observations
        gather_crop([(neg_buffer, ineg)], crop[half:], None, dbs[1])   # negatives: observations
        frames = torch.cat([dbs[0].frames[1], dbs[1].frames[0]], dim=1)   # [n_cam][B][H][W][3]
        rng, key = J.split(rng)
        data = {k: frames[i][:, None] for i, k in enumerate(image_keys)}
        classifier, loss, acc = train_step(classifier, {"data": data, "labels": labels}, key)
        log["pos_idx"].append(ip)
        log["neg_idx"].append(ineg)
        log["crop"].append(crop)
        pending.append((loss, acc))
        if verbose:
            print(f"Epoch: {epoch + 1}, Train Loss: {float(loss):.4f}, Train Accuracy: {float(acc):.4f}")
    log["loss"] = [float(l) for l, _ in pending]
    log["accuracy"] = [float(a) for _, a in pending]
    if classifier_ckpt_path is not None:
        from ..utils.checkpoint import save_checkpoint
        save_checkpoint(classifier_ckpt_path, classifier, step=num_epochs, overwrite=True)
    return classifier, log
