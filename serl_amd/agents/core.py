"""Thin Python handle around the C ABI's `serl_agent` (no numerics here)."""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import Dict, Optional

import numpy as np
import torch

from .. import _lib
from .._handle import Handle
from .._lib_agent import (APPLY_ACTOR_TEMP, APPLY_CRITIC, MLP_SITES, NET_BITS, TX_INDEX, SerlAgentCfg, SerlInfo,  # noqa: F401
                          SerlMlpNoise, SerlNoise)

from ..utils.init import FIXED_STD, NetSpec

TX_NAMES = ("actor", "critic", "temperature")


class AgentCore(Handle):
    prefix = "serl_agent"

    def __init__(self, *, device=0, n_cam, H, W, state_dim, act_dim, batch, ensemble=10, hidden=256,
                 bottleneck=256, sle_features=8, proprio_dim=64, warmup_steps=0, discount=0.96,
                 tau=0.005, lr=3e-4, dropout=0.1, std_min=1e-5, std_max=5.0, target_entropy=None,
                 seed=0, temp_warmup_steps=-1, optimizers=None, encoder_type="resnet-pretrained",
                 critic_subsample_size=2, backup_entropy=False, num_stack=1, std_parameterization="exp",
                 tanh_squash_distribution=True, critic_activation="tanh", policy_activation="tanh",
                 critic_dropout=0.0, policy_dropout=0.0, critic_dims=None, policy_dims=None, critic_layer_norm=True,
                 policy_layer_norm=True, fixed_std=None, ragged=False, use_proprio=True):
        """optimizers: optional {"actor"|"critic"|"temperature": make_optimizer kwargs (common/optimizers.py:6-13:
        learning_rate, warmup_steps, cosine_decay_steps, weight_decay, clip_grad_norm)} overriding lr / warmup_steps.
        weight_decay decays every leaf of the tree, as optax.adamw does with the params the reference hands it -- with
        encoder_type="resnet-pretrained" the pretrained trunk too (`live_trunk`): the reference's behaviour, not a recommendation.
        num_stack: T, frames per observation (SmallEncoder only); state_dim is then the flattened width T * S.
        std_parameterization / tanh_squash_distribution: the policy distribution (Policy's kwargs of the same names).
        critic_activation / policy_activation: one of MLP_ACTIVATIONS each (MLP's `activations`, utils.init.mlp_activations).
        critic_dropout / policy_dropout: MLP's `dropout_rate` in [0, 1) (mlp.py:27-28, utils.init.mlp_dropout_rates); the update's
        losses draw, the evaluation calls (sample_actions, eval_q, eval_policy) never do.
        critic_dims / policy_dims: MLP's `hidden_dims` of each network, 1 to MAX_MLP_LAYERS widths (utils.init.mlp_layer_dims);
        with either given `hidden` stands only for a list left out.  The attributes of the same names read (hidden, hidden) on a
        core made without them.
        critic_layer_norm / policy_layer_norm: MLP's `use_layer_norm` of each network (mlp.py:29-30, utils.init.mlp_layer_norms).
        fixed_std: with std_parameterization="fixed" (and only then) the float32 vector of act_dim finite positive entries that
        utils.init.policy_mode_fixed returns; the head then has no std leaf.  The attribute of the same name reads it back from the
        library (None for another mode).
        ragged: serl_agent_opts.ragged_widths -- hidden and the entries of critic_dims / policy_dims are any integers in [1, 1024];
        a layer off the 64 grid is stored zero padded to the next multiple of 64 (include/serl_mi355.h), and every leaf this handle
        gets, sets or counts has its true shape.
        use_proprio: False is serl_agent_opts.no_proprio (pixel agents alone): EncodingWrapper(use_proprio=False), the image codes
        alone -- no enc/proprio/* leaf, and no call of this handle reads a state: the state tensors of a batch and of
        sample_actions / q_values / policy_stats are accepted and never dereferenced.
        These network options are no fields of serl_agent_cfg: they make one utils.init.NetSpec (`spec`), whose check() says where
        a positive Dropout rate is served, and go to serl_agent_create_opts as one struct (_create)."""
        if target_entropy is None:
            target_entropy = -act_dim / 2
        self.cfg = SerlAgentCfg(device, n_cam, H, W, state_dim, act_dim, batch, ensemble, hidden,
                                bottleneck, sle_features, proprio_dim, warmup_steps, temp_warmup_steps, discount, tau,
                                lr, dropout, std_min, std_max, target_entropy, seed)
        self.cfg.encoder_type = {"resnet-pretrained": 0, "small": 1}[encoder_type]
        # sac.py:150-161: None = the minimum runs over the whole target ensemble
        if critic_subsample_size is not None and not (1 <= int(critic_subsample_size) <= 16):
            raise ValueError(f"critic_subsample_size must be None or in [1, 16] (got {critic_subsample_size})")
        self.cfg.critic_subsample_size = -1 if critic_subsample_size is None else int(critic_subsample_size)
        self.cfg.backup_entropy = 1 if backup_entropy else 0
        self.cfg.num_stack = int(num_stack)
        if (std_parameterization == FIXED_STD) != (fixed_std is not None):
            raise ValueError(f"std_parameterization={std_parameterization!r} with fixed_std={fixed_std!r}: 'fixed' and fixed_std go together")
        if fixed_std is not None:
            v = np.asarray(fixed_std, np.float32).reshape(-1)
            if v.shape != (act_dim,) or not (np.isfinite(v).all() and (v > 0).all()):
                raise ValueError(f"fixed_std must be {act_dim} finite positive numbers (got {fixed_std!r})")
            fixed_std = tuple(float(x) for x in v)
        for name, flag in (("critic_layer_norm", critic_layer_norm), ("policy_layer_norm", policy_layer_norm)):
            if not isinstance(flag, (bool, np.bool_)):
                raise TypeError(f"{name} must be a bool (got {flag!r})")
        if not isinstance(use_proprio, (bool, np.bool_)):
            raise TypeError(f"use_proprio must be a bool (got {use_proprio!r})")
        use_proprio = bool(use_proprio)
        self.spec = NetSpec(std_parameterization, bool(tanh_squash_distribution), fixed_std, critic_activation, policy_activation,
                            float(critic_dropout), float(policy_dropout), int(hidden),
                            None if critic_dims is None else tuple(int(d) for d in critic_dims),
                            None if policy_dims is None else tuple(int(d) for d in policy_dims),
                            bool(critic_layer_norm), bool(policy_layer_norm), bool(ragged), use_proprio)
        opts = self.spec.to_c()      # (an unknown std_parameterization or activation name raises here)
        self.spec.check()
        for f in dataclasses.fields(self.spec):      # the options as public attributes, under the constructor's names ...
            if f.name not in ("hidden", "fixed_std", "critic_dims", "policy_dims"):
                setattr(self, f.name, getattr(self.spec, f.name))
        self.critic_dims, self.policy_dims = self.spec.dims      # ... the two lists resolved
        self._std_param, self._acts = opts.std_param, (opts.critic.act, opts.policy.act)      # SERL_STD_* / SERL_ACT_* codes
        for name, kw in (optimizers or {}).items():
            i = TX_INDEX[name]
            bad = set(kw) - {"learning_rate", "warmup_steps", "cosine_decay_steps", "weight_decay", "clip_grad_norm"}
            if bad:
                raise TypeError(f"make_optimizer() got unexpected keyword arguments {sorted(bad)}")
            if kw.get("learning_rate") is not None:
                self.cfg.tx_lr[i], self.cfg.tx_lr_set[i] = float(kw["learning_rate"]), 1
            if kw.get("warmup_steps") is not None:
                self.cfg.tx_warmup[i] = int(kw["warmup_steps"]) + 1
            if kw.get("cosine_decay_steps") is not None:
                self.cfg.tx_cosine_steps[i] = int(kw["cosine_decay_steps"])
            if kw.get("weight_decay") is not None:
                self.cfg.tx_weight_decay_on[i], self.cfg.tx_weight_decay[i] = 1, float(kw["weight_decay"])
            if kw.get("clip_grad_norm") is not None:
                self.cfg.tx_clip_norm[i] = float(kw["clip_grad_norm"])
        self.device = torch.device("cuda", device)
        super().__init__(self.cfg)
        self._keep = None
        self._snapshots = {}    # (SERL_SNAP_* mask, slots) -> agents/snapshot.py SnapshotHandle
        self._layouts = {}      # leaf -> serl_agent_leaf_layout's five numbers (leaf_layout)

    def __del__(self):
        # the library refuses to destroy an agent that has live snapshot handles
        for h in getattr(self, "_snapshots", {}).values():
            h.close()
        super().__del__()

    def _create(self, cfg):
        return self.L.serl_agent_create_opts(C.byref(cfg), C.byref(self.spec.to_c()), C.byref(self._h))

    # ---- parameters ------------------------------------------------------------------------
    @property
    def leaves(self) -> Dict[str, int]:
        """{leaf: element count}"""
        return self._counts

    def leaf_layout(self, leaf: str):
        """(n, rows, cols, rows_p, ld) of serl_agent_leaf_layout: the leaf is n blocks of rows x cols elements inside n blocks of
        rows_p x ld floats of storage, what serl_agent_grad_view and a snapshot expose; the floats outside the box are zero."""
        if leaf not in self._layouts:      # fixed at creation: asked for once per leaf
            out = (C.c_int64 * 5)()
            _lib.check(self.L.serl_agent_leaf_layout(self._h, leaf.encode(), out))
            self._layouts[leaf] = tuple(int(x) for x in out)
        return self._layouts[leaf]

    @property
    def pad_max_abs(self) -> float:
        """the largest |value| in the padding of the ragged layout over parameters, target parameters, Adam moments and gradients
        (debug tap "pad_max_abs"): exactly 0.0 at every quiescent point"""
        out = np.zeros(1, np.float32)
        _lib.check(self.L.serl_agent_debug_get(self._h, b"pad_max_abs", out.ctypes.data_as(C.POINTER(C.c_float)), 1))
        return float(out[0])

    @property
    def fixed_std(self) -> Optional[np.ndarray]:
        """float32[act_dim]: the fixed_std of a std_parameterization="fixed" agent as the library holds it (before the clip to
        [std_min, std_max], which the head kernels apply); None for an agent of another std parameterisation."""
        if self.spec.fixed_std is None:
            return None
        out = np.zeros(self.cfg.act_dim, np.float32)
        _lib.check(self.L.serl_agent_fixed_std(self._h, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def set_trunk_mode(self, mode: str):
        """'f32' = exact fp32 MFMA convs, 'f16x3' = split-fp16 convs (default)."""
        _lib.check(self.L.serl_agent_set_trunk_mode(self._h, {"f32": 0, "f16x3": 1}[mode]))

    def set_chain_budget(self, workgroups: int):
        """Scheduling hint (no effect on results): workgroup budget of the update's K-split GEMM launches, 0 = default."""
        _lib.check(self.L.serl_agent_set_chain_budget(self._h, int(workgroups)))

    def load_flat(self, section: str, tree: Dict[str, np.ndarray]):
        for k, v in tree.items():
            self.set(section, k, v)

    @property
    def live_trunk(self) -> bool:
        """True for the pretrained ResNet-10 under a non-zero weight_decay in any optimizer: adamw decays the whole tree, the
        "frozen" trunk included (common/optimizers.py:39-42), so the online and the target trunk move at every step and the
        library recomputes the features after each (serl_mi355.h, LIVE TRUNK).  Such a core computes its trunk passes inside the
        update phases: encode_slot only binds the batch, one slot is all a schedule can use, bind_slot is refused."""
        return int(self.L.serl_agent_live_trunk(self._h)) == 1

    @property
    def step(self):
        return int(self.L.serl_agent_get_step(self._h))

    @step.setter
    def step(self, v):
        _lib.check(self.L.serl_agent_set_step(self._h, int(v)))

    # ---- updates ---------------------------------------------------------------------------
    def _noise(self, noise: Optional[dict]):
        """noise: dict of torch device tensors (eps_*, mask_*), np.int32 redq_idx and / or jax.random keys (key_eps_* uint32[..., 2],
        key_mask_* uint32[..., n_cam, 2]: draws made inside the consuming kernels where the tensor is absent), or None.
        The MLPs' Dropout draws ride in the same dict, per site of _lib_agent.MLP_SITES: drop_mask_<site> device u8[2, batch, hidden]
        keep-masks or drop_key_<site> uint32[(update,) 2, 2] keys; they are bound to the agent here, for the call this noise is
        built for (serl_agent_set_mlp_noise)."""
        if noise is None:
            self._keep = None
            return None
        keep = []
        m = None
        if any(k.startswith("drop_") for k in noise):
            m = SerlMlpNoise()
            for i, site in enumerate(MLP_SITES):
                t, k = noise.get("drop_mask_" + site), noise.get("drop_key_" + site)
                if t is not None:
                    t = t.to(device=self.device, dtype=torch.uint8).contiguous()
                    rows = m.mask_rows if m.mask_rows else int(t.shape[1]) if t.dim() == 3 else -1
                    if tuple(t.shape) != (2, rows, self.cfg.hidden):
                        raise ValueError(f"drop_mask_{site}: expected u8[2, batch, {self.cfg.hidden}], the same batch at every site, "
                                         f"got {tuple(t.shape)}")
                    m.mask_rows = rows
                    keep.append(t)
                    m.mask[i] = t.data_ptr()
                if k is not None:
                    k = np.ascontiguousarray(k, dtype=np.uint32)
                    keep.append(k)
                    m.key[i] = k.ctypes.data

        def dev(name, dtype):
            t = noise.get(name)
            if t is None:
                return None
            t = t.to(device=self.device, dtype=dtype).contiguous()
            keep.append(t)
            return t.data_ptr()

        redq = noise.get("redq_idx")
        rp = None
        if redq is not None:
            redq = np.ascontiguousarray(redq, dtype=np.int32)
            keep.append(redq)
            rp = redq.ctypes.data
        def key(name):      # jax.random keys of draws whose tensor is absent (host uint32 words, kept alive with the struct)
            k = noise.get(name)
            if k is None:
                return None
            k = np.ascontiguousarray(k, dtype=np.uint32)
            keep.append(k)
            return k.ctypes.data

        n = SerlNoise(dev("eps_next", torch.float32), dev("mask_next", torch.uint8), rp,
                      dev("eps_pi", torch.float32), dev("mask_obs_pi", torch.uint8),
                      dev("eps_temp", torch.float32), dev("mask_next_temp", torch.uint8),
                      key("key_eps_next"), key("key_mask_next"), key("key_eps_pi"), key("key_mask_obs_pi"),
                      key("key_eps_temp"), key("key_mask_next_temp"))
        self._keep = (keep, n, m)
        # bound last, once nothing above can raise any more: the call this noise goes to consumes the binding
        if m is not None:
            _lib.check(self.L.serl_agent_set_mlp_noise(self._h, C.byref(m)))
        return C.byref(n)

    def update_critics(self, batch, noise=None):
        _lib.check(self.L.serl_agent_update_critics(self._h, C.byref(batch.cstruct), self._noise(noise), self._stream()))

    def update_high_utd(self, batch, utd_ratio=1, noise=None):
        _lib.check(self.L.serl_agent_update_high_utd(self._h, C.byref(batch.cstruct), utd_ratio,
                                                     self._noise(noise), self._stream()))

    def update(self, batch, networks=("actor", "critic", "temperature"), noise=None):
        """SACAgent.update (sac.py:243-299): every selected loss at the same parameters, one optimizer step."""
        bits = 0
        for n in networks:
            bits |= NET_BITS[n]
        _lib.check(self.L.serl_agent_update(self._h, C.byref(batch.cstruct), bits, self._noise(noise), self._stream()))

    def read_info(self) -> dict:
        info = SerlInfo()
        _lib.check(self.L.serl_agent_read_info(self._h, C.byref(info), self._stream()))
        return {n: getattr(info, n) for n, _ in SerlInfo._fields_}

    # ---- reward labelling inside update_critics / update_high_utd (vice.py:546,594) ---------
    reward_classifier = None      # the attached classifier handle (kept alive here: the library borrows it)
    reward_label_mode = None      # None | "features" (head on the slot's trunk features) | "frames" (the classifier's own trunk)

    def set_reward_classifier(self, classifier, cam_of=()):
        """classifier: a serl_classifier Handle, None detaches; cam_of[k] = the agent camera classifier camera k reads."""
        mode = C.c_int()
        if classifier is None:
            _lib.check(self.L.serl_agent_set_reward_classifier(self._h, None, None, C.byref(mode)))
        else:
            _lib.check(self.L.serl_agent_set_reward_classifier(self._h, classifier._h, (C.c_int * len(cam_of))(*cam_of), C.byref(mode)))
        self.reward_classifier = classifier
        self.reward_label_mode = {0: None, 1: "features", 2: "frames"}[mode.value]
        return self.reward_label_mode

    def label_rewards(self):
        """Phase API: label the selected batch (after select_slot / encode); the critic phases then read the labels."""
        _lib.check(self.L.serl_agent_label_rewards(self._h, self._stream()))

    def read_reward_labels(self):
        """-> (labels f32[rows], logits f32[rows], mean label) of the last labelling; synchronises the stream."""
        n = int(self.L.serl_agent_reward_label_rows(self._h))
        lab, lg, mean = np.empty(max(n, 1), np.float32), np.empty(max(n, 1), np.float32), C.c_float()
        _lib.check(self.L.serl_agent_read_reward_labels(self._h, lab.ctypes.data, lg.ctypes.data, C.byref(mean), self._stream()))
        return lab[:n], lg[:n], float(mean.value)

    # ---- data-parallel phases --------------------------------------------------------------
    def set_shard(self, global_offset: int, global_batch: int):
        """This agent's batches are rows [global_offset, ...) of a global batch: device noise is indexed globally."""
        _lib.check(self.L.serl_agent_set_shard(self._h, int(global_offset), int(global_batch)))

    def begin_update(self):
        _lib.check(self.L.serl_agent_begin_update(self._h, self._stream()))

    def encode(self, batch):
        _lib.check(self.L.serl_agent_encode(self._h, C.byref(batch.cstruct), self._stream()))

    def encode_slot(self, batch, slot):
        _lib.check(self.L.serl_agent_encode_slot(self._h, C.byref(batch.cstruct), slot, self._stream()))

    def encode_slot_range(self, batch, slot, stage_begin, stage_end):
        """A piece of encode_slot: stages [stage_begin, stage_end], -1 = conv_init + max-pool, 0..3 = residual stages."""
        _lib.check(self.L.serl_agent_encode_slot_range(self._h, C.byref(batch.cstruct), slot, stage_begin, stage_end, self._stream()))

    def select_slot(self, slot):
        _lib.check(self.L.serl_agent_select_slot(self._h, slot))

    def bind_slot(self, batch, slot):
        """attach a batch to a pipeline slot without running the trunk (its features arrive from another GPU: slot_features)"""
        _lib.check(self.L.serl_agent_bind_slot(self._h, C.byref(batch.cstruct), slot))

    def slot_features(self, slot) -> torch.Tensor:
        """zero-copy view of the slot's frozen-trunk features, f32[2 * n_cam * batch * h*w * 512]"""
        p, n = C.c_void_p(), C.c_int64()
        _lib.check(self.L.serl_agent_slot_features(self._h, slot, C.byref(p), C.byref(n)))
        return _wrap_device_f32(p.value, int(n.value), self.device)

    def critic_grads(self, offset, count, global_count, noise=None, redq_row=0):
        _lib.check(self.L.serl_agent_critic_grads(self._h, offset, count, global_count, self._noise(noise),
                                                  redq_row, self._stream()))

    def critic_grads_bucketed(self, offset, count, global_count, noise=None, redq_row=0, event=None):
        """critic_grads with bucket 0 ([ensemble | head | proprio (none in an image-only agent) | scalars]) published early: `event` (torch.cuda.Event) is
        recorded on the current stream once that bucket is final, before the encoder-head backward is issued."""
        ev = None
        if event is not None:
            if not event.cuda_event:        # lazily created by torch: materialise the hipEvent_t handle
                event.record(torch.cuda.current_stream(self.device))
            ev = C.c_void_p(event.cuda_event)
        _lib.check(self.L.serl_agent_critic_grads_bucketed(self._h, offset, count, global_count, self._noise(noise),
                                                           redq_row, self._stream(), ev))

    def grad_bucket(self, bucket) -> torch.Tensor:
        """Zero-copy view of gradient bucket 0 / 1 (see critic_grads_bucketed); bucket 1 is empty for state-only agents."""
        p, n = C.c_void_p(), C.c_int64()
        _lib.check(self.L.serl_agent_grad_bucket(self._h, bucket, C.byref(p), C.byref(n)))
        return _wrap_device_f32(p.value, int(n.value), self.device) if n.value else torch.empty(0, device=self.device)

    def actor_grads(self, global_count, noise=None):
        _lib.check(self.L.serl_agent_actor_grads(self._h, global_count, self._noise(noise), self._stream()))

    def apply(self, which, info_weight=1.0):
        _lib.check(self.L.serl_agent_apply(self._h, which, info_weight, self._stream()))

    def grad_view(self, which) -> torch.Tensor:
        """The contiguous [grads | scalars] (critic) or [scalars | grads] (actor) device range as a
        torch tensor (zero-copy) for torch.distributed.all_reduce."""
        p, n = C.c_void_p(), C.c_int64()
        _lib.check(self.L.serl_agent_grad_view(self._h, which, C.byref(p), C.byref(n)))
        return _wrap_device_f32(p.value, int(n.value), self.device)

    # ---- misc --------------------------------------------------------------------------------
    def trunk_forward(self, frames_u8: torch.Tensor) -> torch.Tensor:
        n = frames_u8.shape[0]
        H, W = self.cfg.H, self.cfg.W
        fh = fw = None
        h, w = H, W
        for _ in range(5):
            h, w = (h + 1) // 2, (w + 1) // 2
        out = torch.empty((n, h, w, 512), dtype=torch.float32, device=self.device)
        _lib.check(self.L.serl_agent_trunk_forward(self._h, frames_u8.contiguous().data_ptr(), n,
                                                   out.data_ptr(), self._stream()))
        return out

    def sample_actions(self, frames_u8, state, eps=None):
        n = state.shape[0]
        out = torch.empty((n, self.cfg.act_dim), dtype=torch.float32, device=self.device)
        _lib.check(self.L.serl_agent_sample_actions(
            self._h, None if frames_u8 is None else frames_u8.contiguous().data_ptr(), state.contiguous().data_ptr(), n,
            None if eps is None else eps.contiguous().data_ptr(), out.data_ptr(), self._stream()))
        return out

    # ---- read-only evaluation (serl_mi355.h: no byte of the training state is written) ---------
    @staticmethod
    def _ptr(t):
        return None if t is None else t.contiguous().data_ptr()

    def eval_q(self, frames_u8, state, actions, target=False) -> torch.Tensor:
        """forward_critic(obs, actions, train=False), or with target_params -> f32[ensemble, n] (device).  frames_u8
        u8[n_cam, n, (T,) H, W, 3] or None (state-only), state f32[n, T*S], actions f32[n, A]: device tensors, n <= cfg.batch."""
        n = state.shape[0]
        out = torch.empty((self.cfg.ensemble, n), dtype=torch.float32, device=self.device)
        keep = [None if frames_u8 is None else frames_u8.contiguous(), state.contiguous(), actions.contiguous()]
        _lib.check(self.L.serl_agent_eval_q(self._h, self._ptr(keep[0]), keep[1].data_ptr(), keep[2].data_ptr(), n,
                                            1 if target else 0, out.data_ptr(), self._stream()))
        return out

    def eval_policy(self, frames_u8, state, actions=None) -> Dict[str, torch.Tensor]:
        """forward_policy(obs, train=False) -> {"mean": loc, "std": scale_diag, "mode"} f32[n, A] and, with actions,
        "log_prob" f32[n] (device).  A row whose action has a component |a| >= 1 under the tanh squash is not finite."""
        n, A = state.shape[0], self.cfg.act_dim
        out = {k: torch.empty((n, A), dtype=torch.float32, device=self.device) for k in ("mean", "std", "mode")}
        if actions is not None:
            out["log_prob"] = torch.empty((n,), dtype=torch.float32, device=self.device)
        keep = [None if frames_u8 is None else frames_u8.contiguous(), state.contiguous(),
                None if actions is None else actions.contiguous()]
        _lib.check(self.L.serl_agent_eval_policy(self._h, self._ptr(keep[0]), keep[1].data_ptr(), self._ptr(keep[2]), n,
                                                 out["mean"].data_ptr(), out["std"].data_ptr(), out["mode"].data_ptr(),
                                                 self._ptr(out.get("log_prob")), self._stream()))
        return out

    def eval_losses(self, batch, noise=None) -> dict:
        """loss_fns(batch) evaluated, not applied: the scalars and learning rates update(batch, noise=noise) would report."""
        info = SerlInfo()
        _lib.check(self.L.serl_agent_eval_losses(self._h, C.byref(batch.cstruct), self._noise(noise), C.byref(info), self._stream()))
        return {n: getattr(info, n) for n, _ in SerlInfo._fields_}

    def debug(self, what: str, count: int) -> np.ndarray:
        out = np.empty(count, np.float32)
        _lib.check(self.L.serl_agent_debug_get(self._h, what.encode(), out.ctypes.data, count))
        return out


    def trunk_plan(self) -> dict:
        """Kernels the last split-fp16 trunk pass selected: {"images", "pool", "raw_b0", "<layer>": (kernel, cfg, pmode, fused,
        (low-side SAME pad of the rows, of the columns))}."""
        buf = C.create_string_buffer(2048)      # (the library refuses a buffer the text does not fit in)
        _lib.check(self.L.serl_agent_trunk_plan(self._h, buf, 2048))
        out = {}
        for tok in buf.value.decode().split():
            k, v = tok.split("=")
            if "/" in v:
                kern, cfg, pm, fz, pd = v.split("/")
                out[k] = (kern, int(cfg), int(pm), int(fz[1:]), tuple(int(v) for v in pd[1:].split("x")))
            else:
                out[k] = int(v)
        return out

    def debug_set(self, what: str, value):
        v = np.ascontiguousarray(np.asarray(value, dtype=np.float32).reshape(-1))
        _lib.check(self.L.serl_agent_debug_set(self._h, what.encode(), v.ctypes.data, v.size))


class _DevPtr:
    """Minimal __cuda_array_interface__ carrier so torch can alias library-owned HBM."""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (ptr, False), "version": 3}


def _wrap_device_f32(ptr, n, device):
    return torch.as_tensor(_DevPtr(ptr, n), device=device)
