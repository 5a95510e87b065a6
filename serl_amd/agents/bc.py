"""Behaviour cloning with the reference's names (serl_launcher/agents/continuous/bc.py, utils/launcher.py:26-47):

    make_bc_agent(seed, sample_obs, sample_action, image_keys, encoder_type="resnet-pretrained") -> BCAgent
    agent.update(batch) -> (agent, {"actor_loss", "mse"})                    (bc.py:37-77)
    agent.sample_actions(observations, seed=, temperature=, argmax=)         (bc.py:79-97)
    agent.get_debug_metrics(batch) -> {"mse", "log_probs", "pi_actions"}     (bc.py:99-116)

Forward, loss, backward and Adam run in libserl_mi355.so (csrc/bc.hip); no CPU fallback.  `state.rng` advances as
common.py:197-209 does (new_rng, k = split(rng); the loss splits k again for its Dropout key), and the Dropout keep-masks are
drawn inside the SLE kernel from jax.random's threefry under the per-camera keys flax's make_rng gives (serl_amd/jaxrng.py):
a learner started from the same seed draws the masks a JAX learner draws.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, Optional

import numpy as np
import torch

from .. import _lib
from .. import jaxrng as J
from .._handle import Handle, LazyInfo
from .._lib_agent import SerlBcCfg, SerlBcOpts
from ..data.data_store import LazyBatch, gather_crop
from .batch import DeviceBatch
from .flax_tree import AdamTrainState, bc_paths, bc_shapes, leaves_from_tree, trunk_from_flax, tree_from_leaves

SLE_DIM = 512 * 8


class BCTrainState(AdamTrainState):
    """agent.state: JaxRLTrainState-shaped (common.py:81-114), materialised from HBM on access.  BC has ONE optimizer
    over the whole tree, so `opt_states` is optax.adam's tuple (ScaleByAdamState(count, mu, nu), EmptyState()); the
    moments of every frozen leaf are exact zeros.  target_params equals params (BC never updates a target)."""

    fields = ("step", "params", "target_params", "opt_states", "rng")
    opt_field = "opt_states"
    replace_error = TypeError
    opt_states = property(AdamTrainState.adam_state)

    def __init__(self, agent):
        self._a = agent

    @property
    def step(self):
        return int(self._a.L.serl_bc_get_step(self._a._h))

    def _set_step(self, step):
        _lib.check(self._a.L.serl_bc_set_step(self._a._h, step))

    @property
    def params(self):
        return self._export("params")

    @property
    def target_params(self):
        return self.params

    @property
    def rng(self):
        return self._a._rng_key.copy()

    def load_state_dict(self, sd: dict):
        super().load_state_dict(sd)
        if sd.get("rng") is not None:
            self._a._rng_key = np.asarray(sd["rng"], np.uint32).reshape(2).copy()
        return self._a

    def _export(self, section):
        a = self._a
        shapes = bc_shapes(a.image_keys, a.H, a.W, a.S, a.A, use_proprio=a.use_proprio)
        return tree_from_leaves(bc_paths(a.image_keys, a.use_proprio), shapes, lambda leaf: a.get(section, leaf))

    def _import(self, tree, section):
        a = self._a
        paths = bc_paths(a.image_keys, a.use_proprio)
        # a state of the other kind (with / without the proprio branch under `encoder`) is refused whole, before any leaf is written
        enc = tree.get("modules_actor", {}).get("encoder") if isinstance(tree, dict) else None
        if isinstance(enc, dict) and ("Dense_0" in enc or "LayerNorm_0" in enc) != a.use_proprio:
            raise ValueError(f"{section}: the state was written by a BC agent with use_proprio={not a.use_proprio} ('modules_actor/encoder/"
                             f"Dense_0' is {'present' if not a.use_proprio else 'absent'}), this agent has use_proprio={a.use_proprio}; "
                             "nothing was loaded")
        for leaf, v in leaves_from_tree(paths, tree):
            v = np.asarray(v, np.float32)
            if section != "params" and not a._trainable[leaf]:
                if np.any(v):
                    raise ValueError(f"{section} of the frozen leaf {'/'.join(paths[leaf])} is not zero")
                continue
            a.set(section, leaf, v)


class _Info(LazyInfo):
    """The info dict of one update: {'actor_loss', 'mse'}, copied on the device when the update is issued and read on
    first access (no host synchronisation per step)."""

    def __init__(self, dev):
        self._dev = dev

    def _read(self):
        v = self._dev.cpu().numpy()
        return {"actor_loss": float(v[0]), "mse": float(v[1])}

    def __len__(self):   # known without reading the device
        return 2


class BCAgent(Handle):
    prefix = "serl_bc"

    def __init__(self, image_keys, H, W, state_dim, act_dim, *, seed_key, max_batch=256, learning_rate=3e-4, device=0,
                 dropout=0.1, std_min=1e-5, std_max=5.0, use_proprio=True):
        if not isinstance(use_proprio, (bool, np.bool_)):
            raise TypeError(f"use_proprio must be a bool (got {use_proprio!r})")
        self.use_proprio = bool(use_proprio)     # False: serl_bc_opts.no_proprio, the image codes alone; the state is never read
        self.image_keys = tuple(image_keys)
        self.H, self.W, self.S, self.A, self.max_batch, self.device = H, W, state_dim, act_dim, max_batch, device
        self.config = {"image_keys": self.image_keys, "use_proprio": self.use_proprio}
        super().__init__(SerlBcCfg(device, len(self.image_keys), H, W, state_dim, act_dim, max_batch, learning_rate, dropout,
                                   std_min, std_max))
        self._rng_key = J.create_rng(seed_key)    # BCAgent.create (bc.py:194-202)
        self._db: Optional[DeviceBatch] = None
        self.state = BCTrainState(self)

    def _create(self, cfg):
        return self.L.serl_bc_create_opts(C.byref(cfg), C.byref(SerlBcOpts(0 if self.use_proprio else 1)), C.byref(self._h))

    # ------------------------------------------------------------------ construction (bc.py:118-204)
    @classmethod
    def create(cls, rng, observations, actions, encoder_type: str = "small", image_keys: Iterable[str] = ("image",),
               use_proprio: bool = False, network_kwargs: dict = None, policy_kwargs: dict = None,
               learning_rate: float = 3e-4, batch_size: int = 256, device: int = 0, param_seed: Optional[int] = None,
               param_init: str = "numpy"):
        """`rng`: a jax.random key (uint32[2]) or an int seed.  Only the frozen pretrained ResNet-10 encoder is served.
        As for DrQAgent.create_drq, the trunk keeps its initialiser's values until the caller runs
        utils.train_utils.load_resnet10_params(agent, image_keys) (the reference calls it at the end of create, bc.py:200-203,
        and downloads the pickle when it is absent; there is no download here).
        use_proprio: False (the reference's default, bc.py:126) is EncodingWrapper(use_proprio=False): the policy reads the
        concatenated camera codes alone, `encoder` holds no Dense_0 / LayerNorm_0, network/Dense_0's kernel is (256 * n_cam, 256),
        and only the two MLP layers and the two heads train.  observations["state"] is still required (the stores carry it); its
        values are never read.  True adds the proprio branch (what make_bc_agent builds).
        param_init: "numpy" (default) or "reference" (the reference's own initialisers and keys from `rng`, utils/init_ref.py)."""
        from ..utils import init_ref
        reference = init_ref.check_param_init(param_init)
        if encoder_type != "resnet-pretrained":
            raise ValueError(f"encoder_type {encoder_type!r}: only 'resnet-pretrained' is implemented for BC on this library")
        if not isinstance(use_proprio, (bool, np.bool_)):
            raise ValueError(f"use_proprio={use_proprio!r}: True or False")
        nk = dict(network_kwargs or {"hidden_dims": [256, 256]})
        if list(nk.get("hidden_dims", [256, 256])) != [256, 256] or nk.get("use_layer_norm", False) or \
                nk.get("activations", "tanh") not in ("tanh", None) and getattr(nk.get("activations"), "__name__", "") != "tanh":
            raise ValueError(f"network_kwargs {nk}: only MLP([256, 256], tanh, no LayerNorm) is implemented")
        pk = dict(policy_kwargs or {"tanh_squash_distribution": False})
        if pk.get("tanh_squash_distribution", False) or pk.get("std_parameterization", "exp") != "exp":
            raise ValueError(f"policy_kwargs {pk}: only the un-squashed Gaussian with exp std is implemented")
        key = J.prngkey(int(rng)) if np.ndim(rng) == 0 else np.asarray(rng, np.uint32).reshape(2)
        image_keys = tuple(image_keys)
        img = np.asarray(observations[image_keys[0]])
        H, W = img.shape[-3], img.shape[-2]
        S = int(np.asarray(observations["state"]).shape[-1])
        A = int(np.asarray(actions).shape[-1])
        agent = cls(image_keys, H, W, S, A, seed_key=key, max_batch=batch_size, learning_rate=learning_rate, device=device,
                    std_min=float(pk.get("std_min", 1e-5)), std_max=float(pk.get("std_max", 10.0)), use_proprio=bool(use_proprio))
        from ..utils.init import init_theta, init_trunk
        seed = int(key[1]) if param_seed is None else param_seed
        agent.load_flat(init_trunk(seed))
        if reference:
            theta = init_ref.bc_reference(image_keys, H, W, S, A, key, device=device, use_proprio=agent.use_proprio)
        else:
            theta = init_theta(len(image_keys), H, W, S, A, seed=seed, use_proprio=agent.use_proprio)
        agent.load_flat({k: v for k, v in theta.items() if k in agent._counts})
        return agent

    # ------------------------------------------------------------------ flat leaves
    def leaves(self, trainable: Optional[bool] = None):
        return [k for k in self._counts if trainable is None or self._trainable[k] == trainable]

    def load_flat(self, flat: Dict[str, np.ndarray], section: str = "params"):
        """flat: trunk leaves, 'enc/<camera index or image key>/...', 'enc/proprio/...', 'actor/...'."""
        for name, v in flat.items():
            if name.startswith("enc/") and not name.startswith("enc/proprio"):
                _, k, leaf = name.split("/", 2)
                if k in self.image_keys:
                    name = f"enc/{self.image_keys.index(k)}/{leaf}"
            self.set(section, name, v)
        return self

    def load_trunk_params(self, pretrained: Dict[str, dict]):
        """utils/train_utils.py:69-130 on the BC tree: the pickle's {conv_init, norm_init, ResNetBlock_i} into the trunk."""
        return self.load_flat(trunk_from_flax(pretrained))

    # ------------------------------------------------------------------ batches
    def _device_batch(self, B):
        if B > self.max_batch:
            raise ValueError(f"batch {B} > max_batch {self.max_batch} (BCAgent.create(batch_size=...))")
        if self._db is None or self._db.batch != B:
            self._db = DeviceBatch(B, len(self.image_keys), self.H, self.W, 3, self.S, self.A, self.device)
        return self._db

    def prepare(self, batch) -> DeviceBatch:
        """A replay sample -> DeviceBatch (only the observation half is consumed): LazyBatch through the fused gather with no
        crop (the augmentation is commented out in bc.py:41-44); a reference-format dict, packed ([B, 2, H, W, 3]: _unpack,
        bc.py:39-40) or unpacked ([B, 1, H, W, 3] / [B, H, W, 3]), by device copies."""
        if isinstance(batch, DeviceBatch):
            return batch
        if isinstance(batch, LazyBatch):
            db = self._device_batch(batch.batch_size)
            gather_crop(batch.parts, None, None, db)
            return db
        obs = batch["observations"]
        B = int(batch["actions"].shape[0])
        db = self._device_batch(B)
        dev = db.frames.device
        for i, k in enumerate(self.image_keys):
            v = torch.as_tensor(obs[k], device=dev)
            if v.dim() == 5:
                v = v[:, 0]
            db.frames[0, i].copy_(v.reshape(B, self.H, self.W, 3))
        db.state[0].copy_(torch.as_tensor(obs["state"], device=dev).reshape(B, self.S))
        db.action.copy_(torch.as_tensor(batch["actions"], device=dev).reshape(B, self.A))
        return db

    # ------------------------------------------------------------------ bc.py:37-77
    def update_keys(self, rng=None):
        """(new state.rng, per-camera Dropout keys) of one update from state.rng (common.py:197-209, bc.py:46-54)"""
        rng = self._rng_key if rng is None else np.asarray(rng, np.uint32)
        new_rng, k = J.split(rng)
        key = J.split(k)[1]
        return new_rng, np.stack([J.flax_make_rng(key, J.dropout_path(c)) for c in self.image_keys]).astype(np.uint32)

    def update(self, batch, pmap_axis: str = None, masks: Optional[Dict[str, np.ndarray]] = None):
        """masks: optional injected Dropout keep-masks {image key: u8[B, 4096]} (parity tests); by default they are drawn
        from jax.random keys inside the SLE kernel."""
        if pmap_axis is not None:
            raise NotImplementedError("pmap_axis: multi-GPU BC is not implemented")
        db = self.prepare(batch)
        new_rng, cam_keys = self.update_keys()
        mptr, keep = None, None
        if masks is not None:
            keep = torch.stack([torch.as_tensor(np.asarray(masks[k], np.uint8)).reshape(db.batch, SLE_DIM) for k in self.image_keys])
            keep = keep.to(db.frames.device).contiguous()
            mptr = C.c_void_p(keep.data_ptr())
        keys = np.ascontiguousarray(cam_keys.reshape(-1), np.uint32)
        s = self._stream()
        _lib.check(self.L.serl_bc_update(self._h, C.byref(db.cstruct), mptr, keys.ctypes.data_as(C.c_void_p), s))
        info = torch.empty(2, dtype=torch.float32, device=db.frames.device)
        _lib.check(self.L.serl_bc_read_info(self._h, C.c_void_p(info.data_ptr()), s))
        self._rng_key = new_rng
        self._keep_masks = keep   # (alive until the stream has consumed it)
        return self, _Info(info)

    # ------------------------------------------------------------------ bc.py:79-97
    def _obs(self, observations):
        """-> (frames u8[n_cam][n][H][W][3], state f32[n][S], batched).  enable_stacking: an image of 5 dims is [B, T, H, W, C],
        of 4 dims one observation [T, H, W, C] (encoding.py:38-42); T must be 1."""
        st = np.asarray(observations["state"].cpu() if torch.is_tensor(observations["state"]) else observations["state"], np.float32)
        img0 = observations[self.image_keys[0]]
        batched = len(img0.shape) == 5
        n = int(img0.shape[0]) if len(img0.shape) == 5 else 1
        frames = []
        for k in self.image_keys:
            v = torch.as_tensor(observations[k]).to(torch.device("cuda", self.device))
            frames.append(v.reshape(n, self.H, self.W, 3))
        f = torch.stack(frames).contiguous()
        s = torch.from_numpy(np.ascontiguousarray(st.reshape(n, self.S))).to(f.device)
        return f, s, batched

    def sample_actions(self, observations, *, seed=None, temperature: float = 1.0, argmax: bool = False):
        f, s, batched = self._obs(observations)
        n = f.shape[1]
        if n > self.max_batch:
            raise ValueError(f"{n} observations > max_batch {self.max_batch}")
        out = torch.empty((n, self.A), dtype=torch.float32, device=f.device)
        eps_ptr, key_ptr, keep = None, None, None
        if not argmax:
            if seed is None:
                raise ValueError("sample_actions: a seed is needed unless argmax=True")
            if torch.is_tensor(seed) and seed.is_floating_point() or (isinstance(seed, np.ndarray) and seed.dtype.kind == "f"):
                keep = torch.as_tensor(seed, dtype=torch.float32).reshape(n, self.A).to(f.device).contiguous()   # injected eps
                eps_ptr = C.c_void_p(keep.data_ptr())
            else:
                keep = np.ascontiguousarray(np.asarray(seed, np.uint32).reshape(2))
                key_ptr = keep.ctypes.data_as(C.c_void_p)
        _lib.check(self.L.serl_bc_sample_actions(self._h, C.c_void_p(f.data_ptr()), C.c_void_p(s.data_ptr()), n, eps_ptr, key_ptr,
                                                 float(temperature), 1 if argmax else 0, C.c_void_p(out.data_ptr()), self._stream()))
        a = out.cpu().numpy()
        return a if batched else a[0]

    # ------------------------------------------------------------------ bc.py:99-116
    def get_debug_metrics(self, batch, **kwargs):
        db = self.prepare(batch)
        B, dev = db.batch, db.frames.device
        mse = torch.empty(B, dtype=torch.float32, device=dev)
        logp = torch.empty(B, dtype=torch.float32, device=dev)
        pi = torch.empty((B, self.A), dtype=torch.float32, device=dev)
        _lib.check(self.L.serl_bc_debug_metrics(self._h, C.byref(db.cstruct), C.c_void_p(mse.data_ptr()), C.c_void_p(logp.data_ptr()),
                                                C.c_void_p(pi.data_ptr()), self._stream()))
        return {"mse": mse.cpu().numpy(), "log_probs": logp.cpu().numpy(), "pi_actions": pi.cpu().numpy()}

    def replace(self, **kw):
        if "state" in kw and kw["state"] is not self.state:
            self.state.load_state_dict(kw["state"].state_dict() if hasattr(kw["state"], "state_dict") else kw["state"])
        return self


def make_bc_agent(seed, sample_obs, sample_action, image_keys=("image",), encoder_type="resnet-pretrained",
                  batch_size=256, device=0, param_init="numpy", use_proprio=True):
    """launcher.py:26-47 (hyper-parameters copied from there).  The reference's default encoder_type "small" raises at this
    reference commit; only "resnet-pretrained" is served here."""
    return BCAgent.create(
        J.prngkey(seed), sample_obs, sample_action,
        network_kwargs={"activations": "tanh", "use_layer_norm": False, "hidden_dims": [256, 256]},
        policy_kwargs={"tanh_squash_distribution": False, "std_parameterization": "exp", "std_min": 1e-5, "std_max": 5},
        use_proprio=use_proprio, encoder_type=encoder_type, image_keys=image_keys, batch_size=batch_size, device=device,
        param_init=param_init)
