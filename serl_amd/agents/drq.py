"""DrQAgent / SACAgent with the reference's Python API, backed by libserl_mi355.so.

Mirrors (same names, argument meaning, error behaviour):
  serl_launcher/agents/continuous/drq.py:24-328   DrQAgent.create_drq / update_high_utd / update_critics
  serl_launcher/agents/continuous/sac.py:243-320  SACAgent.update / sample_actions
  serl_launcher/common/common.py:81-114           JaxRLTrainState fields (step, params, target_params,
                                                   opt_states, rng) exposed through `agent.state`
The reference is functional (returns a new agent); this agent mutates its device state and
returns `self`, which is what the learner loop (`agent, info = agent.update_critics(batch)`) needs.
All numerics run in HIP kernels; there is no CPU fallback.
"""
from __future__ import annotations

from typing import Dict, FrozenSet, Iterable, Optional

import numpy as np
import torch

from ..data.data_store import LazyBatch, gather_crop
from ..utils import init as pinit
from ..utils import init_ref
from .. import _lib
from .. import jaxrng as J
from .._handle import LazyInfo
from ..call_noise import CallNoise
from .batch import DeviceBatch
from .core import APPLY_ACTOR_TEMP, APPLY_CRITIC, TX_NAMES, AgentCore
from .flax_tree import export_tree


def lr_schedule(kw: dict, count: int) -> float:
    """make_optimizer's learning-rate schedule (common/optimizers.py:14-30) at `count`."""
    import math
    peak, warm = float(kw.get("learning_rate", 3e-4)), int(kw.get("warmup_steps", 0) or 0)
    if count < warm:
        return peak * count / warm
    cos = kw.get("cosine_decay_steps")
    if cos is not None:
        T = max(int(cos) - warm, 1)
        return peak * 0.5 * (1.0 + math.cos(math.pi * min(count - warm, T) / T))
    return peak


class PendingInfo(LazyInfo):
    """Info dict of the LAST update call; reading it synchronises the stream (the reference's jitted
    update returns device arrays that are also only materialised when logged)."""

    def __init__(self, agent, kind, serial, labelled=False):
        self._agent, self._kind, self._serial, self._labelled = agent, kind, serial, labelled

    def _read(self) -> dict:
        if self._agent._update_serial != self._serial:
            raise RuntimeError("info of an older update was overwritten; read it before the next update")
        r = self._agent.core.read_info()
        lr = {f"{n}_lr": r[f"{n}_lr"] for n in TX_NAMES}
        if isinstance(self._kind, frozenset):   # SACAgent.update: an info dict per network, {} for the skipped ones
            nets = self._kind
            out = {"critic": {k: r[k] for k in ("critic_loss", "predicted_qs", "target_qs")} if "critic" in nets else {},
                   "actor": {k: r[k] for k in ("actor_loss", "temperature", "entropy")} if "actor" in nets else {},
                   "temperature": {"temperature_loss": r["temperature_loss"]} if "temperature" in nets else {}}
        else:
            out = {"critic": {k: r[k] for k in ("critic_loss", "predicted_qs", "target_qs")}}
            if self._kind == "high_utd":
                out["actor"] = {k: r[k] for k in ("actor_loss", "temperature", "entropy")}
                out["temperature"] = {"temperature_loss": r["temperature_loss"]}
                if self._labelled:     # vice.py:609: info["vice_rewards"] = rewards.mean()
                    out["vice_rewards"] = self._agent.core.read_reward_labels()[2]
        out.update(lr)
        return out


def opt_states_tree(agent, step, export) -> dict:
    """{tx: InjectHyperparamsState} in flax's state-dict form (flax.serialization.to_state_dict: NamedTuples become
    dicts of their fields, tuples dicts keyed '0', '1', ...).  Each reference tx is
    optax.inject_hyperparams(chain([clip_by_global_norm], adam | adamw)) (common/optimizers.py:32-56):
      {count, hyperparams: {learning_rate}, inner_state: {'0': <clip: {}>?, '<k>': {'0': {count, mu, nu}, '1': {} ...}}}
    (non-numeric hyper-parameters such as weight_decay=None are not stored by optax).  `step`: the count and the point of the
    learning-rate schedule; export(section) -> the flax tree of "opt/<tx>/mu" / "opt/<tx>/nu"."""
    out = {}
    step = np.int32(step)
    for tx in TX_NAMES:
        kw = agent._opts.get(tx, {})
        adam = {"count": step, "mu": export(f"opt/{tx}/mu"), "nu": export(f"opt/{tx}/nu")}
        # optax.adam = chain(scale_by_adam, scale_by_learning_rate); adamw adds add_decayed_weights in between
        inner_adam = {"0": adam, "1": {}} if kw.get("weight_decay") is None else {"0": adam, "1": {}, "2": {}}
        stages = ([{}] if kw.get("clip_grad_norm") is not None else []) + [inner_adam]
        hp = {"learning_rate": np.float32(agent.lr_at(int(step), tx))}
        if kw.get("weight_decay") is not None:
            hp["weight_decay"] = np.float32(kw["weight_decay"])
        out[tx] = {"count": step, "hyperparams": hp, "inner_state": {str(i): s for i, s in enumerate(stages)}}
    return out


class TrainStateView:
    """agent.state: JaxRLTrainState-shaped, materialised from HBM on access (common.py:81-114)."""

    def __init__(self, agent):
        self._a = agent

    @property
    def step(self):
        return self._a.core.step

    @property
    def params(self):
        return export_tree(self._a.core, "params", self._a.image_keys)

    @property
    def target_params(self):
        return export_tree(self._a.core, "target_params", self._a.image_keys)

    @property
    def opt_states(self):
        return opt_states_tree(self._a, self._a.core.step, lambda section: export_tree(self._a.core, section, self._a.image_keys))

    @property
    def rng(self):
        return self._a._rng_key.copy()

    def replace(self, **kw):
        """JaxRLTrainState.replace(params=..., target_params=..., opt_states=..., step=...): loads the given trees
        into HBM (in place) and returns the view."""
        bad = set(kw) - {"params", "target_params", "opt_states", "step", "rng"}
        if bad:
            raise TypeError(f"unknown TrainState fields: {sorted(bad)}")
        from ..utils.checkpoint import load_state_dict
        load_state_dict(self._a, {k: v for k, v in kw.items() if k != "rng"})
        if kw.get("rng") is not None:
            self._a._rng_key = np.asarray(kw["rng"], np.uint32).copy()
        return self


class DrQAgent:
    _DRQ_AUG = True     # update_critics / update_high_utd open with `rng, obs_rng, next_obs_rng = split(rng, 3)` (drq.py:276-277,307-308)

    def __init__(self, core: AgentCore, image_keys, config: dict, seed: int):
        self.core = core
        self.image_keys = tuple(image_keys)
        self.config = config
        self.num_stack = max(int(core.cfg.num_stack), 1)     # T, frames per observation (ChunkingWrapper(obs_horizon=T))
        self._np_rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([seed, 0xD1CE])))
        # RANDOMNESS.  "threefry" (default): the reference's own stream -- crop offsets, REDQ indices, policy noise and Dropout
        # masks are drawn from jax.random's threefry2x32 with the reference's key schedule (serl_amd/jaxrng.py), and `state.rng`
        # advances as common.py:197-209 / sac.py:287-289 / drq.py:276-318 do: a learner started from the same seed consumes the
        # numbers a JAX learner consumes (integers bit-exact).  "hash": crop offsets from a numpy PCG64 stream, noise hashed on
        # the device from cfg.seed inside the kernels that use it (no noise tensors; what the bench's DataParallelLearner runs).
        self.rng_impl = "threefry"
        # how the threefry draws reach the kernels: "keys" = the kernels draw them in place from the call's keys (no noise tensors,
        # no extra launch); "tensors" = one serl_jax_fill launch per call materialises them (bit-identical results:
        # tests/test_drq_agent_gpu.py; the tensors can then be inspected -- agent._noise_bufs); serl_amd/call_noise.py builds both
        self.noise_form = "keys"
        self._rng_key = J.create_rng(seed)     # state.rng as create_drq / create leave it (drq.py:69-84, sac.py:355-372)
        self.last_draws = {}     # what the last update call drew from its keys (crop offsets, REDQ indices): parity tests read it
        self._call_noise = CallNoise(core, self.image_keys, self.last_draws)
        self._batch: Optional[DeviceBatch] = None
        self._update_serial = 0
        self.state = TrainStateView(self)
        # transparent software pipelining for batches that come from `get_iterator(..., lazy=True)`: the iterator has
        # already sampled the NEXT batch, so its gather + crop + frozen trunk run on a second stream under this update
        self.prefetch = True
        self._sched = None
        self._slot_batches = [None, None, None]   # one device batch per pipeline slot (TorchPipelineSchedule.slots)
        self._slot_crops = [None, None, None]     # the crop offsets drawn for the batch in each slot
        self._prefetched = None   # (key of the lazy batch, slot)

    # ------------------------------------------------------------------ construction
    @classmethod
    def create_drq(cls, rng, observations, actions, encoder_type: str = "small", shared_encoder: bool = True,
                   use_proprio: bool = False, critic_network_kwargs: dict = None,
                   policy_network_kwargs: dict = None, policy_kwargs: dict = None,
                   critic_ensemble_size: int = 2, critic_subsample_size: Optional[int] = None,
                   temperature_init: float = 1.0, image_keys: Iterable[str] = ("image",),
                   discount: float = 0.95, soft_target_update_rate: float = 0.005,
                   target_entropy: Optional[float] = None, backup_entropy: bool = False,
                   batch_size: int = 256, device: int = 0, learning_rate: float = 3e-4,
                   actor_optimizer_kwargs: dict = None, critic_optimizer_kwargs: dict = None,
                   temperature_optimizer_kwargs: dict = None, param_init: str = "numpy", mlp_dropout: bool = False, mlp_shapes: bool = False, mlp_plain: bool = False,
                   policy_fixed: bool = False, mlp_ragged: bool = False, image_only: bool = False, **kwargs):
        """drq.py:104-242.  Only the configuration the reference's examples run is built natively:
        encoder_type="resnet-pretrained", use_proprio=True, REDQ subsample 2, tanh-squashed
        exp-parameterised policy, LayerNorm+tanh MLPs (utils/launcher.py:79-116) -- 256x256 there; critic_network_kwargs /
        policy_network_kwargs may give hidden_dims=[h, h], h a multiple of 64 in [64, 1024], the same in both, and
        activations "tanh" (when absent), "relu" or "swish" / "silu", by name or as a callable of that name, chosen per network
        (mlp.py:19-31); other activations and a positive dropout_rate are refused.  mlp_dropout=True switches MLP Dropout on: a
        dropout_rate (a number below 1) in either network kwargs then puts Dropout in front of that MLP's two LayerNorms
        (mlp.py:27-28; the critic's is DroQ) -- the update's losses draw, acting and evaluation never do.
        mlp_shapes=True reads each network's own hidden_dims instead: 1 to 4 layers, every width a multiple of 64 in [64, 1024], the
        critic's list independent of the policy's (utils.init.mlp_layer_dims; [h, h] in both gives the same agent as without the
        switch; with a positive dropout_rate under mlp_dropout=True only one [h, h] is served).
        mlp_plain=True reads each network's own use_layer_norm (mlp.py:29-30; utils.init.mlp_layer_norms): a network with False has
        no LayerNorm in its MLP -- y = act(Dense(x) + b) per layer, the leaves w<j> and b<j> alone, no LayerNorm_<j> in the flax tree --
        at every activation, depth and width served, with or without mlp_shapes.  An absent key means True, and True in both gives the
        same agent as without the switch.  The encoder's bottleneck and proprio layers keep their LayerNorm.  Together with a
        positive dropout_rate under mlp_dropout=True it is refused.
        policy_kwargs: std_parameterization "exp", "softplus" or "uniform" (one trainable log_stds vector, no Dense_1) and
        tanh_squash_distribution True or False all run in the head kernels; "fixed" is refused.  A key that is absent, or
        policy_kwargs=None, means the launcher's value ("exp", True).
        policy_fixed=True also reads std_parameterization="fixed" with fixed_std (utils.init.policy_mode_fixed), how the reference
        writes TD3 (sac.py:23-28): fixed_std is a scalar, broadcast, or action_dim numbers, each finite and positive, and
        stds = clip(fixed_std, std_min, std_max) in every row.  The head then has no std parameter at all -- no Dense_1 and no
        log_stds in the flax tree, the optimizer state or a checkpoint; agent.config["fixed_std"] holds the vector, which a
        checkpoint does not carry.  fixed_std beside another std_parameterization, "fixed" without fixed_std (ValueError, as in the
        reference), another length and a non-finite or non-positive entry are refused from the arguments alone; so is a
        positive dropout_rate under mlp_dropout=True beside it.  Any other mode under the switch gives the agent the call
        without the switch gives.
        mlp_ragged=True: every width that hidden_dims carries, with or without mlp_shapes, is any integer in [1, 1024] (mlp.py:19-31
        takes any list; TD3's and DDPG's published [400, 300]) at every depth, activation and use_layer_norm served.  A layer off the
        64 grid is stored zero padded to the next multiple of 64 on the device; params, target_params, opt_states, checkpoints and
        snapshots have the true shapes.  Widths on the grid give the agent the call without the switch gives.  A positive
        dropout_rate under mlp_dropout=True beside a width off the grid is refused.
        Frame stacks: the sample observation carries T = observations[image_key].shape[0] frames and a (T, S) state, as
        ChunkingWrapper(obs_horizon=T) produces them; EncodingWrapper(enable_stacking=True) folds them into the channels and the
        proprio width (common/encoding.py:39-44,58-64).  T in 1..4 with encoder_type="small"; the pretrained ResNet-10 cannot take
        a stack (its conv_init kernel has 3 input channels).
        {actor,critic,temperature}_optimizer_kwargs: make_optimizer's (common/optimizers.py:6-13).  weight_decay selects
        optax.adamw, which decays EVERY leaf of the tree it is given (optimizers.py:39-42) -- with encoder_type="resnet-pretrained"
        that includes the pretrained trunk, which then shrinks by sum_t lr_t * wd_t per optimizer step while its target copy
        follows by the EMA (`agent.live_trunk`; costs a third trunk pass, re-packed weights per step and the prefetch overlap:
        DESIGN.md section 7).  That is what the reference computes, and it is reproduced for parity -- not a recommendation.
        image_only=True reads use_proprio as given (without the switch use_proprio=False, the reference's own default, is refused as
        it always was).  False builds EncodingWrapper(use_proprio=False) (common/encoding.py:53-72): the code is the concatenated
        camera codes, there is no Dense_0 / LayerNorm_0 under either `encoder` in the flax tree, the first kernels of the critic
        and the policy have 256 * n_cam (+ action_dim) rows, and the update launches no proprio work.  observations["state"] is still
        required in the sample observation and in every batch, because the replay stores carry it; its values are never read.
        True gives the agent the call without the switch gives.  A use_proprio that is no bool, and a positive dropout_rate under
        mlp_dropout=True beside use_proprio=False, are refused from the arguments alone.  agent.config holds "use_proprio": False
        for such an agent (no entry otherwise).
        param_init: "numpy" (default) draws the trainable leaves from host NumPy streams seeded by `rng`; "reference" draws them
        as the reference's model_def.init(init_rng) does (utils/init_ref.py); the frozen trunk is the same either way."""
        if encoder_type not in ("resnet-pretrained", "small"):
            # drq.py:155-167 also has "resnet" (trainable ResNet-10, never selected by an example: not built)
            raise NotImplementedError(f"Unknown encoder type: {encoder_type}")
        if image_only:
            if not isinstance(use_proprio, (bool, np.bool_)):
                raise NotImplementedError(f"use_proprio={use_proprio!r} under image_only=True (served: True or False)")
        elif not use_proprio:
            raise NotImplementedError("only use_proprio=True; the image-only agent (use_proprio=False) with image_only=True")
        pk = policy_kwargs or {}
        A = int(np.asarray(actions).shape[-1])
        spec = pinit.network_spec(critic_network_kwargs, policy_network_kwargs, pk, A, mlp_dropout=mlp_dropout, mlp_shapes=mlp_shapes,
                                  mlp_plain=mlp_plain, policy_fixed=policy_fixed, mlp_ragged=mlp_ragged,
                                  use_proprio=bool(use_proprio) if image_only else True)
        seed = int(np.asarray(rng).reshape(-1)[-1]) if not isinstance(rng, int) else rng
        image_keys = tuple(image_keys)
        img = np.asarray(observations[image_keys[0]])
        H, W = img.shape[-3], img.shape[-2]
        st0 = np.asarray(observations["state"])
        T = int(img.shape[-4]) if img.ndim >= 4 else 1
        if T > 1:
            if st0.ndim < 2 or st0.shape[-2] != T:
                raise ValueError(f"observations[{image_keys[0]!r}] stacks {T} frames, observations['state'] has shape {st0.shape}: "
                                 f"expected ({T}, S)")
            if encoder_type == "resnet-pretrained":
                raise NotImplementedError(
                    f"num_stack {T} with encoder_type='resnet-pretrained': the stack is folded into {3 * T} channels "
                    "(common/encoding.py:39-44) and the pretrained ResNet-10's conv_init kernel (7,7,3,64) takes 3; "
                    "use encoder_type='small'")
        S = int(st0.shape[-1]) * T      # the proprio Dense's input: "B T S -> B (T S)" (common/encoding.py:58-64)
        if target_entropy is None:
            target_entropy = -A / 2  # drq.py:88-89
        # drq.py:35-43: each optimizer = make_optimizer(learning_rate=3e-4) unless overridden (optimizers.py:6-13)
        opts = {"actor": {"learning_rate": learning_rate, **(actor_optimizer_kwargs or {})},
                "critic": {"learning_rate": learning_rate, **(critic_optimizer_kwargs or {})},
                "temperature": {"learning_rate": learning_rate, **(temperature_optimizer_kwargs or {})}}
        core = AgentCore(device=device, n_cam=len(image_keys), H=H, W=W, state_dim=S, act_dim=A,
                         batch=batch_size, ensemble=critic_ensemble_size, discount=discount,
                         tau=soft_target_update_rate, lr=learning_rate, std_min=pk.get("std_min", 1e-5),
                         std_max=pk.get("std_max", 10.0), target_entropy=target_entropy, seed=seed,
                         optimizers={k: {"warmup_steps": 0, **v} for k, v in opts.items()}, encoder_type=encoder_type,
                         critic_subsample_size=critic_subsample_size, backup_entropy=backup_entropy, num_stack=T,
                         **spec.core_kwargs())
        if init_ref.check_param_init(param_init):
            theta = init_ref.theta_reference(image_keys, H, W, S, A, rng, ensemble=critic_ensemble_size, encoder_type=encoder_type,
                                             temperature_init=temperature_init, device=device, num_stack=T, **spec.leaf_kwargs())
        else:
            theta = pinit.init_theta(len(image_keys), H, W, S, A, seed=seed, temperature_init=temperature_init,
                                     ensemble=critic_ensemble_size, encoder_type=encoder_type, num_stack=T, **spec.leaf_kwargs())
        trunk = pinit.init_trunk(seed=seed) if encoder_type == "resnet-pretrained" else {}
        for sec in ("params", "target_params"):  # JaxRLTrainState.create(target_params=params)
            core.load_flat(sec, theta)
            core.load_flat(sec, trunk)
        config = dict(critic_ensemble_size=critic_ensemble_size, critic_subsample_size=critic_subsample_size,
                      discount=discount, soft_target_update_rate=soft_target_update_rate,
                      target_entropy=target_entropy, backup_entropy=backup_entropy, image_keys=image_keys, **spec.config_entries())
        agent = cls(core, image_keys, config, seed)
        agent._opts = {k: {"warmup_steps": 0, **v} for k, v in opts.items()}
        if param_init == "reference":
            agent._rng_key = J.create_rng(rng)
        return agent

    def snapshot(self, sections=("params",), slots=3):
        """A consistent copy of the selected TrainState fields ("params", "target_params", "opt_states") as they are once every
        update enqueued so far has run, taken in one kernel launch on the stream the updates run on and moved to pinned host
        memory behind the learner's back: agents/snapshot.py StateSnapshot.  Returns at once; the updates that follow are not in
        it and do not wait for the copy.  `slots` snapshots (1..4) of one choice of sections can be held at a time -- with every
        slot held the call raises SerlError (status -3); 3, the default, is what publishing needs: one with the publisher thread,
        one queued behind it, one being taken.  The handle is created at the first call and reused by later calls with the same
        arguments.
            server.publish_network(agent.snapshot)      # async_drq_sim.py:295-297; the server takes it: never raises when behind
            save_checkpoint(path, agent.snapshot(("params", "target_params", "opt_states")), step=...)   # :303-307"""
        from .snapshot import take_snapshot
        return take_snapshot(self, sections, slots)

    @property
    def live_trunk(self) -> bool:
        """True when an optimizer's weight_decay reaches the pretrained trunk (AgentCore.live_trunk): the trunk then decays at
        every optimizer step, its target copy follows by the EMA, every step is followed by fresh trunk passes on the update
        stream, `prefetch` has no effect, and an attached reward classifier labels from its own trunk ("frames")."""
        return self.core.live_trunk

    def lr_at(self, count, tx="critic"):
        """optimizers.py:14-30: warm-up -> constant, or warm-up -> cosine decay."""
        return lr_schedule(self._opts[tx], count)

    def load_trunk_params(self, pretrained: Dict[str, dict]):
        """utils/train_utils.py:69-130: patch the frozen ResNet-10 trunk from the pretrained pickle's
        tree {conv_init: {kernel}, norm_init: {scale,bias}, ResNetBlock_i: {...}} (params and target)."""
        from .flax_tree import trunk_from_flax
        flat = trunk_from_flax(pretrained)
        for sec in ("params", "target_params"):
            self.core.load_flat(sec, flat)
        return self

    def replace(self, **kw):
        """agent.replace(state=...) of the reference (e.g. `agent.replace(state=restored_ckpt)`).  The state is
        device-resident here: a flax-layout dict (or this agent's own state view) is loaded into HBM in place."""
        if kw and set(kw) - {"state"}:
            raise NotImplementedError(list(kw))
        st = kw.get("state")
        if isinstance(st, dict):
            from ..utils.checkpoint import load_state_dict
            load_state_dict(self, st)
        elif st is not None and st is not self.state:
            raise TypeError("state must be a flax-layout dict (params / target_params / opt_states / step) or agent.state")
        return self

    # ------------------------------------------------------------------ learned rewards (vice.py:546,594)
    def set_reward_classifier(self, classifier, image_keys=None):
        """Label rewards at update time, as VICEAgent.update_critics / update_high_utd do (vice.py:546,594): with a classifier
        attached (serl_amd.networks.reward_classifier.Classifier; None detaches) those two calls replace the batch's rewards by
        (sigmoid(classifier(augmented next_obs, train=False)) >= 0.5) * 1.0, once per call over the whole batch; `update` keeps the
        stored rewards (VICE does not override it).  Neither the caller's batch nor the replay store is written, and no random
        number is drawn.  update_high_utd's info gains "vice_rewards", the mean label (vice.py:609).
        image_keys: the agent camera each classifier camera reads, by name, in the classifier's camera order (default: the
        classifier's own image_keys) -- a subset of the agent's, in any order.
        The classifier's head runs on the frozen-trunk features the update already holds when both trunks are bit-identical
        (reward_label_mode "features", compared here), else its own trunk runs on the augmented next frames ("frames"; always with
        a live trunk, which is the classifier's only until the first optimizer step; the optimizer's own changes of it never
        make the attachment stale).  Setting a
        trunk leaf on either side afterwards (load_trunk_params) makes the next labelled update raise until this is called again.
        Train the classifier with its train_step between updates, on the stream the updates run on."""
        if classifier is None:
            self.core.set_reward_classifier(None)
            return self
        if not self.image_keys:
            raise _lib.SerlError("a state-only agent has no frames for a reward classifier to label")
        keys = tuple(classifier.image_keys if image_keys is None else image_keys)
        if len(keys) != len(classifier.image_keys):
            raise _lib.SerlError(f"the classifier has {len(classifier.image_keys)} cameras, image_keys names {len(keys)}")
        lacking = [k for k in keys if k not in self.image_keys]
        if lacking:
            raise _lib.SerlError(f"the reward classifier reads {lacking}, which are not among the agent's image_keys {self.image_keys}")
        self.core.set_reward_classifier(classifier, [self.image_keys.index(k) for k in keys])
        return self

    @property
    def reward_classifier(self):
        return self.core.reward_classifier

    @property
    def reward_label_mode(self):
        """None (no classifier attached), "features" or "frames": see set_reward_classifier"""
        return self.core.reward_label_mode

    def last_reward_labels(self):
        """(labels, logits) f32[batch] of the last labelled update, rows in batch order; synchronises the stream"""
        lab, lg, _ = self.core.read_reward_labels()
        return lab, lg

    def _label_slot(self):
        """the label phase of the pipelined path: the slot is selected, its features (or frames) are ready"""
        if self.core.reward_classifier is not None:
            self.core.label_rewards()

    # ------------------------------------------------------------------ batches
    def _device_batch(self, B):
        c = self.core.cfg
        if self._batch is None or self._batch.batch != B:
            self._batch = DeviceBatch(B, c.n_cam, c.H, c.W, 3, c.state_dim, c.act_dim, c.device, self.num_stack)
        return self._batch

    def _draw_crops(self, B, rng=None):
        """data_augmentation_fn (drq.py:244-253): one (dy, dx) in [0, 8] per frame, the SAME for every camera; obs and next_obs
        use independent keys (drq.py:279-281).  A stack of T frames draws B*T offsets per stream, entry b*T + t for frame t of
        sample b: batched_random_crop(num_batch_dims=2) flattens to B*T images and splits its key B*T ways.  `rng`: state.rng at the entry of the call that consumes the batch (None: the
        current one) -- rng, obs_rng, next_obs_rng = split(rng, 3); offsets = batched_random_crop's (data_augmentations.py:22-36)."""
        n = B * self.num_stack
        if self.rng_impl != "threefry":
            co = self._np_rng.integers(0, 9, size=(n, 2)).astype(np.int32)
            cn = self._np_rng.integers(0, 9, size=(n, 2)).astype(np.int32)
            return co, cn
        return J.crop_pair(self._rng_key if rng is None else rng, n)

    # ------------------------------------------------------------------ the reference's random stream for one call
    def _call_keys(self, n_critic, has_actor_temp, drq_aug=None, combined=False):
        """Keys of the learner call about to run, derived from state.rng (None when the device-hashed stream is selected)."""
        if self.rng_impl != "threefry":
            return None
        return J.UpdateKeys(self._rng_key, self._DRQ_AUG if drq_aug is None else drq_aug, n_critic, has_actor_temp, combined,
                            self._subsample_none)

    @property
    def _subsample_none(self):
        """UpdateKeys' last argument: None without MLP Dropout (the keys the agent always derived), else whether
        critic_subsample_size is None -- the online critic's Dropout rng then equals the target critic's (sac.py:143-176)"""
        if self.core.critic_dropout <= 0 and self.core.policy_dropout <= 0:
            return None
        return int(self.core.cfg.critic_subsample_size) < 0

    @property
    def _noise_bufs(self):
        """{batch: the noise tensors of the last call} under noise_form = "tensors" (serl_amd/call_noise.py)"""
        return self._call_noise.bufs

    def _run_call(self, keys, kind, noise, rows, run, **want):
        """What every update method ends with: the call's noise -- the injected one, else drawn from the call's keys (None with
        the device-hashed stream) -- goes to `run`; state.rng then advances as the reference's and the info becomes readable."""
        if noise is None and keys is not None:
            noise = self._call_noise.build(keys, rows, self.noise_form, **want)
        run(noise)
        if keys is not None:
            self._rng_key = keys.rng_out.copy()
        self._update_serial += 1
        labelled = kind in ("critics", "high_utd") and self.core.reward_classifier is not None
        return self, PendingInfo(self, kind, self._update_serial, labelled)

    def prepare(self, batch, crops=None) -> DeviceBatch:
        """sample-gather [+ concat_batches] + _unpack + random-shift crop -> DeviceBatch."""
        if isinstance(batch, DeviceBatch):
            return batch
        if isinstance(batch, LazyBatch):
            B = batch.batch_size
            if self.core.cfg.n_cam > 0 and batch.num_stack != self.num_stack:
                raise ValueError(f"the batch comes from a store of stacks of {batch.num_stack} frames, this agent was built for "
                                 f"num_stack {self.num_stack}")
            out = self._device_batch(B)
            co, cn = crops if crops is not None else self._draw_crops(B)
            self.last_draws["crop_obs"], self.last_draws["crop_next"] = co, cn
            gather_crop(batch.parts, co, cn, out)
            return out
        # reference-format dict of device tensors (packed or unpacked frames)
        import ctypes as C
        obs, nobs = batch["observations"], batch["next_observations"]
        B = int(batch["rewards"].shape[0])
        out = self._device_batch(B)
        co, cn = crops if crops is not None else self._draw_crops(B)
        self.last_draws["crop_obs"], self.last_draws["crop_next"] = co, cn
        keep, ptrs, T = [], (C.c_void_p * len(self.image_keys))(), self.num_stack
        for i, k in enumerate(self.image_keys):
            if k in nobs and T == 1:  # unpacked: re-pack [B,2,H,W,C] (train_utils._unpack inverse)
                p = torch.cat([obs[k], nobs[k]], dim=1).contiguous()
            elif k in nobs:           # unpacked stacks [B,T,...]: the window is obs frames 0..T-1 + the last next frame
                if not torch.equal(obs[k][:, 1:], nobs[k][:, :-1]):
                    raise ValueError(f"observations[{k!r}][:, 1:] differs from next_observations[{k!r}][:, :-1]: not the two "
                                     "views of one packed window (train_utils._unpack)")
                p = torch.cat([obs[k][:, :T], nobs[k][:, -1:]], dim=1).contiguous()
            else:
                p = obs[k].contiguous()
            if p.shape[1] != T + 1:
                raise ValueError(f"a packed window of {p.shape[1]} frames under {k!r}: this agent was built for num_stack {T} "
                                 f"({T + 1} frames)")
            keep.append(p)
            ptrs[i] = p.data_ptr()
        c = self.core.cfg
        s = torch.cuda.current_stream(self.core.device).cuda_stream
        _lib.check(_lib.lib().serl_crop_packed_stacked(c.device, ptrs, c.n_cam, B, T, c.H, c.W, 3, co.ctypes.data,
                                                       cn.ctypes.data, out.frames.data_ptr(), C.c_void_p(s)))
        out.state[0].copy_(obs["state"].reshape(B, -1))
        out.state[1].copy_(nobs["state"].reshape(B, -1))
        out.action.copy_(batch["actions"])
        out.reward.copy_(batch["rewards"])
        out.mask.copy_(batch["masks"])
        out._keep = keep
        return out

    # ------------------------------------------------------------------ pipelined acquisition of lazy batches
    @staticmethod
    def _lazy_key(batch: LazyBatch):
        return tuple((id(b), id(ix)) for b, ix in batch.parts)

    def _can_prefetch(self, batch, crops):
        # (only the FROZEN trunk can run ahead of the update: a trainable encoder depends on the parameters, and so does a live
        #  trunk -- a pass of batch i+1 under the update of batch i would read the weights from before that update's apply)
        return (self.prefetch and not self.live_trunk and crops is None and isinstance(batch, LazyBatch) and self.core.cfg.n_cam > 0
                and self.core.cfg.encoder_type == 0 and batch.batch_size <= self.core.cfg.batch)

    def _slot_batch(self, slot, B):
        c = self.core.cfg
        if self._slot_batches[slot] is None or self._slot_batches[slot].batch != B:
            if self._sched is not None:     # the side / gather streams may still be using the buffers about to be freed
                self._sched.side_stream.synchronize()
                if getattr(self._sched, "gather_stream", None) is not None:
                    self._sched.gather_stream.synchronize()
            self._slot_batches[slot] = DeviceBatch(B, c.n_cam, c.H, c.W, 3, c.state_dim, c.act_dim, c.device, self.num_stack)
        return self._slot_batches[slot]

    def _produce(self, batch: LazyBatch, slot, db, rng=None):
        """gather + crop on the schedule's gather stream, the frozen trunk on the side stream.  (Round 2 gathered on the CALLER's
        stream at the moment the pass needed it and made the side stream wait: a dependency that crosses streams and actually
        blocks costs 60-100 us on this stack, at every pass.  Since round 5 the gather of the NEXT batch runs on a third stream while
        the previous pass is still computing -- the side stream's wait is satisfied long before it is reached -- and the pass starts
        at conv_init: parallel.py TorchPipelineSchedule.gathered.  An actor-side insert that overwrites a slot waits ON THE COPY
        STREAM for the gathers in flight, never on the host.)"""
        sch = self._sched
        co, cn = self._draw_crops(db.batch, rng)      # rng: state.rng at the entry of the call that will consume this batch
        self._slot_crops[slot] = (co, cn)
        sch.wait_consumed(slot)     # host side: the update that used this slot ended two passes ago
        with sch.side():
            sch.gathered(slot, lambda: gather_crop(batch.parts, co, cn, db))
            self.core.encode_slot(db, slot)
        sch.produced(slot)

    def _acquire(self, batch: LazyBatch, next_rng=None):
        """-> (slot, DeviceBatch) with the frozen-trunk features of `batch` ready in `slot` (prefetched during the
        previous update, or encoded now), and starts the same work for the iterator's next batch on the side stream.
        `next_rng`: state.rng after the call in progress = at the entry of the call that consumes the next batch (the key
        schedule is pure host arithmetic, so the next batch's crop keys are known before this update has run)."""
        from ..parallel import TorchPipelineSchedule
        if self._sched is None:
            self._sched = TorchPipelineSchedule(self.core.device, prioritise_update=False)
            if self.core.cfg.batch >= 128:
                self.core.set_chain_budget(256)      # the chain now runs beside the trunk pass (see parallel.py)
        sch, B = self._sched, batch.batch_size
        key = self._lazy_key(batch)
        hit = self._prefetched is not None and self._prefetched[0] == key
        if hit and self.rng_impl == "threefry" and self._prefetched[3] is not None \
                and not np.array_equal(self._prefetched[3], self._rng_key):
            # The slot's crop offsets were drawn from the state.rng this call was EXPECTED to enter with.  state.rng moved in
            # between (state.replace(rng=...) after a checkpoint restore / reseed, or an update on a non-lazy batch): the
            # reference would crop with the current key, so the slot is stale -- produce it again.
            hit = False
        if hit:
            slot = self._prefetched[1]
            sch.wait_produced(slot)
            db = self._slot_batches[slot]
        else:
            # not prefetched (first call, or the caller skipped a batch).  All trunk work goes through the side stream,
            # in order: the feature slots share one trunk workspace.
            slot = 0 if self._prefetched is None else (self._prefetched[1] + 1) % sch.slots
            db = self._slot_batch(slot, B)
            self._produce(batch, slot, db)
            sch.wait_produced(slot)
        self.last_draws["crop_obs"], self.last_draws["crop_next"] = self._slot_crops[slot]
        self._prefetched = None
        nxt = batch.peek_next() if batch.peek_next is not None else None
        if nxt is not None and nxt.batch_size == B:
            s2 = (slot + 1) % sch.slots
            self._produce(nxt, s2, self._slot_batch(s2, B), next_rng)
            # (the parts are kept alive with the key: a freed index array's address could otherwise be reused by a
            # later sample and false-match)
            self._prefetched = (self._lazy_key(nxt), s2, list(nxt.parts), None if next_rng is None else np.array(next_rng, np.uint32))
        self.core.select_slot(slot)
        return slot, db

    def _sync_side_stream(self):
        """The non-pipelined paths run the trunk on the caller's stream and share the trunk workspace with a prefetched
        encode_slot that may still be in flight on the side stream: order behind it and drop the prefetch (it would
        otherwise be consumed after its workspace was overwritten)."""
        if self._sched is not None:
            torch.cuda.current_stream(self.core.device).wait_stream(self._sched.side_stream)
            self._prefetched = None

    # ------------------------------------------------------------------ updates
    def update_critics(self, batch, *, pmap_axis: Optional[str] = None, noise=None, crops=None):
        """drq.py:296-328.  `noise` / `crops` inject explicit draws (parity tests); None = drawn from state.rng."""
        keys = self._call_keys(1, False)
        if self._can_prefetch(batch, crops):
            slot, db = self._acquire(batch, None if keys is None else keys.rng_out)

            def run(noise):
                self._label_slot()
                self.core.begin_update()
                self.core.critic_grads(0, db.batch, db.batch, noise)
                self.core.apply(APPLY_CRITIC)
                self._sched.consumed(slot)
        else:
            db = self.prepare(batch, crops)
            self._sync_side_stream()
            run = lambda noise: self.core.update_critics(db, noise)  # noqa: E731
        return self._run_call(keys, "critics", noise, db.batch, run)

    def update_high_utd(self, batch, *, utd_ratio: int, pmap_axis: Optional[str] = None, noise=None, crops=None):
        """drq.py:255-294 -> sac.py:544-596."""
        keys = self._call_keys(utd_ratio, True)
        if self._can_prefetch(batch, crops):
            B = batch.batch_size
            assert B % utd_ratio == 0, f"Batch size {B} must be divisible by UTD ratio {utd_ratio}"  # sac.py:561-563
            slot, db = self._acquire(batch, None if keys is None else keys.rng_out)

            def run(noise):
                mb = B // utd_ratio
                self._label_slot()
                self.core.begin_update()
                for i in range(utd_ratio):
                    self.core.critic_grads(i * mb, mb, mb, noise, i)
                    self.core.apply(APPLY_CRITIC, 1.0 / utd_ratio)
                self.core.actor_grads(B, noise)
                self.core.apply(APPLY_ACTOR_TEMP)
                self._sched.consumed(slot)
        else:
            db = self.prepare(batch, crops)
            assert db.batch % utd_ratio == 0, \
                f"Batch size {db.batch} must be divisible by UTD ratio {utd_ratio}"  # sac.py:561-563
            self._sync_side_stream()
            run = lambda noise: self.core.update_high_utd(db, utd_ratio, noise)  # noqa: E731
        return self._run_call(keys, "high_utd", noise, db.batch, run)

    def update(self, batch, *, pmap_axis: str = None,
               networks_to_update: FrozenSet[str] = frozenset({"actor", "critic", "temperature"}), noise=None):
        """sac.py:243-299 on an already augmented batch: every loss in `networks_to_update` is evaluated at the same
        parameters, all three optimizers step once (zero gradients for the others), target EMA iff "critic" is in the
        set.  Any non-empty subset works, the default (all three) included."""
        loss_keys = {"actor", "critic", "temperature"}
        assert set(networks_to_update).issubset(loss_keys), f"Invalid gradient steps: {networks_to_update}"
        assert len(networks_to_update) > 0, "networks_to_update is empty"
        if isinstance(batch, DeviceBatch):
            db = batch
        else:  # identity crop (offset 4 = centre of the 9 shifts): the batch is taken as already augmented
            n = batch.batch_size if isinstance(batch, LazyBatch) else int(batch["rewards"].shape[0])
            db = self.prepare(batch, crops=(np.full((n * self.num_stack, 2), 4, np.int32),) * 2)
        self._sync_side_stream()
        # SACAgent.update (sac.py:243-299): no augmentation split; every selected loss takes its key from ONE 4-way split
        nets = set(networks_to_update)
        crit, act = "critic" in nets, bool(nets & {"actor", "temperature"})
        keys = self._call_keys(1 if crit else 0, act, drq_aug=False, combined=crit and act)
        return self._run_call(keys, frozenset(networks_to_update), noise, db.batch,
                              lambda noise: self.core.update(db, tuple(networks_to_update), noise), want_critic=crit, want_actor=act)

    # ------------------------------------------------------------------ acting
    def sample_actions(self, observations, *, seed=None, argmax: bool = False, **kwargs):
        """sac.py:301-320: policy forward with train=False; sample (external seed) or mode.  Observations are (T, H, W, 3) frames
        and a (T, S) state per sample (T = num_stack; the T axis of a single-frame agent may be missing), batched or not."""
        if argmax:
            assert seed is None, "Cannot specify seed when sampling deterministically"
        c = self.core.cfg
        st = np.asarray(observations["state"], np.float32)
        batched = st.ndim == 3
        n = st.shape[0] if batched else 1
        fshape = (n,) + ((self.num_stack,) if self.num_stack > 1 else ()) + (c.H, c.W, 3)
        frames = np.stack([np.asarray(observations[k], np.uint8).reshape(fshape) for k in self.image_keys])
        self._sync_side_stream()
        f = torch.from_numpy(frames).to(self.core.device)
        s = torch.from_numpy(st.reshape(n, -1)).to(self.core.device)
        eps = None if argmax else self._action_noise(seed, n)
        a = self.core.sample_actions(f, s, eps).cpu().numpy()
        return a if batched else a[0]

    # ------------------------------------------------------------------ read-only evaluation
    # What the trained networks think, without a step: the reference's forward_critic / forward_target_critic (sac.py:33-69),
    # forward_policy(obs, train=False) with .distribution.loc / .scale_diag / .mode() / .log_prob(a) (sac.py:71-91) and
    # loss_fns(batch) (sac.py:134-241).  None of these calls changes params, target_params, opt_states, step or state.rng, and an
    # update that follows computes what it would have computed without them.
    def _eval_obs(self, observations):
        """host observations in the forms sample_actions accepts -> (frames u8[n_cam, n, (T,) H, W, 3] device, state f32[n, T*S]
        device, n, batched)"""
        c = self.core.cfg
        st = np.asarray(observations["state"], np.float32)
        # (n, T, S) is a batch, (T, S) one observation; a single-frame agent may drop the T axis: (n, S) with n > 1 is then a batch
        batched = st.ndim == 3 or (self.num_stack == 1 and st.ndim == 2 and st.shape[0] > 1)
        n = st.shape[0] if batched else 1
        fshape = (n,) + ((self.num_stack,) if self.num_stack > 1 else ()) + (c.H, c.W, 3)
        frames = np.stack([np.asarray(observations[k], np.uint8).reshape(fshape) for k in self.image_keys])
        return torch.from_numpy(frames).to(self.core.device), torch.from_numpy(st.reshape(n, -1)).to(self.core.device), n, batched

    def _eval_actions(self, actions, n):
        a = np.asarray(actions, np.float32).reshape(n, self.core.cfg.act_dim)
        return torch.from_numpy(a).to(self.core.device)

    def _chunks(self, n):
        """n > cfg.batch is served in chunks of cfg.batch rows"""
        B = int(self.core.cfg.batch)
        return [(lo, min(lo + B, n)) for lo in range(0, n, B)]

    def _q_dev(self, f, s, a, target):
        return torch.cat([self.core.eval_q(None if f is None else f[:, lo:hi], s[lo:hi], a[lo:hi], target)
                          for lo, hi in self._chunks(s.shape[0])], dim=1)

    def _policy_dev(self, f, s, a):
        parts = [self.core.eval_policy(None if f is None else f[:, lo:hi], s[lo:hi], None if a is None else a[lo:hi])
                 for lo, hi in self._chunks(s.shape[0])]
        return {k: torch.cat([p[k] for p in parts], dim=0) for k in parts[0]}

    def q_values(self, observations, actions, *, target: bool = False) -> np.ndarray:
        """forward_critic(observations, actions, train=False) -- with target=True forward_target_critic -> f32[ensemble, n]
        (n = 1 for a single observation)."""
        self._sync_side_stream()
        f, s, n, _ = self._eval_obs(observations)
        return self._q_dev(f, s, self._eval_actions(actions, n), target).cpu().numpy()

    def policy_stats(self, observations, actions=None) -> dict:
        """forward_policy(observations, train=False) -> {"mean": .distribution.loc, "std": .scale_diag, "mode": .mode()} [n, A]
        (without the leading axis for a single observation) and, with `actions`, "log_prob": .log_prob(actions) [n].
        Under the tanh squash an action with a component of exactly +-1 (stored gripper commands often are) has no finite
        atanh and its log_prob is not finite, as in the reference: nothing is clamped here."""
        self._sync_side_stream()
        f, s, n, batched = self._eval_obs(observations)
        out = self._policy_dev(f, s, None if actions is None else self._eval_actions(actions, n))
        out = {k: v.cpu().numpy() for k, v in out.items()}
        return out if batched else {k: v[0] for k, v in out.items()}

    def evaluate_batch(self, batch, *, side: str = "observations") -> dict:
        """The four questions on a replay batch (what `update` takes: a host dict, a DeviceBatch or a LazyBatch of the store --
        gathered in HBM, never through the host) -> {"q", "q_target": [ensemble, B], "mean", "std", "mode": [B, A], "log_prob":
        [B]} at the batch's observations, or with side="next_observations" at its next observations, with the batch's actions.
        Frames are taken as already augmented (the identity crop of `update`)."""
        if side not in ("observations", "next_observations"):
            raise ValueError(f"side must be 'observations' or 'next_observations' (got {side!r})")
        if isinstance(batch, DeviceBatch):
            db = batch
        else:
            n = batch.batch_size if isinstance(batch, LazyBatch) else int(batch["rewards"].shape[0])
            db = self.prepare(batch, crops=(np.full((n * self.num_stack, 2), 4, np.int32),) * 2)
        self._sync_side_stream()
        w = 0 if side == "observations" else 1
        f = db.frames[w] if self.core.cfg.n_cam > 0 else None
        s, a = db.state[w], db.action
        out = {"q": self._q_dev(f, s, a, False), "q_target": self._q_dev(f, s, a, True), **self._policy_dev(f, s, a)}
        return {k: v.cpu().numpy() for k, v in out.items()}

    def evaluate_losses(self, batch, *, noise=None, rng=None) -> dict:
        """loss_fns(batch) evaluated and not applied: the nested info dict `update(batch)` returns -- critic / actor /
        temperature losses and the three learning rates -- at the current parameters, bit for bit what an `update` issued right
        after it with the same noise reports.  noise: explicit draws as in the update calls; rng: a jax.random key to derive
        the call's keys from; with neither they are derived from state.rng, which does not advance."""
        if isinstance(batch, DeviceBatch):
            db = batch
        else:
            n = batch.batch_size if isinstance(batch, LazyBatch) else int(batch["rewards"].shape[0])
            db = self.prepare(batch, crops=(np.full((n * self.num_stack, 2), 4, np.int32),) * 2)
        self._sync_side_stream()
        if noise is None and self.rng_impl == "threefry":
            key = self._rng_key if rng is None else np.asarray(rng, np.uint32)
            keys = J.UpdateKeys(key, False, 1, True, True, self._subsample_none)       # the split of update() with all three networks
            drawn = dict(self.last_draws)     # (last_draws records what the last UPDATE drew: put back below)
            noise = self._call_noise.build(keys, db.batch, self.noise_form, want_critic=True, want_actor=True)
            self.last_draws.clear()
            self.last_draws.update(drawn)
        r = self.core.eval_losses(db, noise)
        out = {"critic": {k: r[k] for k in ("critic_loss", "predicted_qs", "target_qs")},
               "actor": {k: r[k] for k in ("actor_loss", "temperature", "entropy")},
               "temperature": {"temperature_loss": r["temperature_loss"]}}
        out.update({f"{n}_lr": r[f"{n}_lr"] for n in TX_NAMES})
        return out

    def _action_noise(self, seed, n):
        """dist.sample(seed=seed) of sac.py:316-320: distrax draws jax.random.normal(seed, (1,) + batch + (A,))."""
        assert seed is not None, "Must specify rng when sampling"
        c = self.core.cfg
        eps = torch.empty((n, c.act_dim), dtype=torch.float32, device=self.core.device)
        if self.rng_impl == "threefry" and J.is_key(seed):
            J.fill(c.device, [J.job(J.NORMAL, seed, n * c.act_dim, eps.data_ptr())], self.core._stream())
            return eps
        g = np.random.Generator(np.random.PCG64(np.random.SeedSequence(np.asarray(seed).reshape(-1).tolist())))
        return torch.from_numpy(g.standard_normal((n, c.act_dim)).astype(np.float32)).to(self.core.device)
