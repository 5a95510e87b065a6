"""Synthetic parameter initialisation (flax initialisers restated) for the DrQ agent.

The reference initialises with flax (`model_def.init`, agents/continuous/drq.py:69-75) and then
overwrites the ResNet-10 trunk with weights downloaded at run time (utils/train_utils.py:69-130).
Neither flax nor the network is available here, so the trunk gets seeded synthetic weights of the
same tree/shape; real weights are loaded with DrQAgent.load_trunk_params().
Leaf names/shapes = the flat arena of libserl_mi355.so, camera index instead of key.
The trainable leaves here come from host NumPy streams seeded by the integer seed: the default (param_init="numpy") of every
constructor.  param_init="reference" draws the same leaves as the reference's model_def.init(init_rng) does, from jax.random's
threefry stream under flax's per-module keys (utils/init_ref.py); the trunk comes from init_trunk either way.
"""
from __future__ import annotations

import ctypes
import dataclasses
import math
import re
from typing import Optional, Tuple

import numpy as np

STAGES = ((64, 1), (128, 2), (256, 2), (512, 2))


def trunk_shapes():
    sh = {"trunk/conv_init": (7, 7, 3, 64), "trunk/norm_init/scale": (64,), "trunk/norm_init/bias": (64,)}
    cin = 64
    for i, (f, s) in enumerate(STAGES):
        p = f"trunk/block{i}/"
        sh[p + "conv0"] = (3, 3, cin, f)
        sh[p + "gn0/scale"] = (f,)
        sh[p + "gn0/bias"] = (f,)
        sh[p + "conv1"] = (3, 3, f, f)
        sh[p + "gn1/scale"] = (f,)
        sh[p + "gn1/bias"] = (f,)
        if s != 1 or cin != f:
            sh[p + "proj"] = (1, 1, cin, f)
            sh[p + "gnp/scale"] = (f,)
            sh[p + "gnp/bias"] = (f,)
        cin = f
    return sh


def feat_hw(H, W):
    h, w = H, W
    for _ in range(5):
        h, w = (h + 1) // 2, (w + 1) // 2
    return h, w


SMALL_FEATURES = (3, 32, 64, 128, 256)   # SmallEncoder(features=(32, 64, 128, 256)) on RGB (drq.py:140-151)


HIDDEN_WIDTHS = tuple(range(64, 1025, 64))   # serl_agent_cfg.hidden: one wave per LayerNorm row, hidden / 64 columns per lane


RAGGED_WIDTHS = range(1, 1025)   # ... with serl_agent_opts.ragged_widths: a layer off the grid is stored 64 ceil(d / 64) wide, zero padded


_PLAIN_HINT = "; without LayerNorm with mlp_plain=True"


def _is_width(d):
    return not isinstance(d, bool) and isinstance(d, (int, np.integer))


def mlp_hidden_width(critic_network_kwargs=None, policy_network_kwargs=None, mlp_plain=False, mlp_ragged=False) -> int:
    """The one width h of the critic's and the policy's MLPs from the reference's `critic_network_kwargs` /
    `policy_network_kwargs` (hidden_dims=[h, h], LayerNorm, default [256, 256]).  Served: two layers of the same width, the same
    in both networks, a multiple of 64 from 64 to 1024; anything else raises NotImplementedError.  mlp_plain=True (the argument
    of the same name of create_states / create_drq): use_layer_norm is mlp_layer_norms' to read.  mlp_ragged=True (likewise): h is
    any integer in [1, 1024]; 0, a negative, 1025 and a width that is no integer are refused."""
    grid = "any integer in [1, 1024] under mlp_ragged=True" if mlp_ragged else "a multiple of 64 in [64, 1024]"
    served = f"served: hidden_dims=[h, h] with LayerNorm, h {grid}, the same h for critic and policy"
    widths = []
    for which, nk in (("critic_network_kwargs", critic_network_kwargs or {}), ("policy_network_kwargs", policy_network_kwargs or {})):
        if not mlp_plain and not nk.get("use_layer_norm", True):
            raise NotImplementedError(f"{which}: use_layer_norm=False ({served}{_PLAIN_HINT})")
        dims = list(nk.get("hidden_dims", [256, 256]))
        if mlp_ragged and not all(_is_width(d) for d in dims):
            raise NotImplementedError(f"{which}: hidden_dims={dims} holds a width that is no integer ({served})")
        dims = [int(d) for d in dims]
        if len(dims) != 2:
            raise NotImplementedError(f"{which}: hidden_dims={dims} has {len(dims)} layers ({served})")
        if dims[0] != dims[1]:
            raise NotImplementedError(f"{which}: hidden_dims={dims} has two different layer widths ({served})")
        if dims[0] not in (RAGGED_WIDTHS if mlp_ragged else HIDDEN_WIDTHS):
            raise NotImplementedError(f"{which}: width {dims[0]} is {'outside [1, 1024]' if mlp_ragged else 'off the grid'} ({served})")
        widths.append(dims[0])
    if widths[0] != widths[1]:
        raise NotImplementedError(f"critic width {widths[0]} and policy width {widths[1]} differ ({served})")
    return widths[0]


MAX_MLP_LAYERS = 4   # SERL_MAX_MLP_LAYERS


def mlp_layer_dims(critic_network_kwargs=None, policy_network_kwargs=None, mlp_plain=False, mlp_ragged=False):
    """(critic, policy): the `hidden_dims` of the reference's MLP (networks/mlp.py:19-31 loops over a list of any length) from its
    two network kwargs, as tuples of ints: what create_states / create_drq read with mlp_shapes=True (without the switch
    mlp_hidden_width reads and refuses as it always did).  Default [256, 256].  Served: 1 to MAX_MLP_LAYERS layers per network,
    every width a multiple of 64 in [64, 1024], the two lists independent, LayerNorm on; anything else raises NotImplementedError
    from the arguments alone.  mlp_plain=True: use_layer_norm is mlp_layer_norms' to read.  mlp_ragged=True: every width is any
    integer in [1, 1024]."""
    grid = "any integer in [1, 1024] under mlp_ragged=True" if mlp_ragged else "a multiple of 64 in [64, 1024]"
    served = (f"served: hidden_dims of 1 to {MAX_MLP_LAYERS} layers with LayerNorm, every width {grid}, "
              "the critic's list independent of the policy's")
    out = []
    for which, nk in (("critic_network_kwargs", critic_network_kwargs or {}), ("policy_network_kwargs", policy_network_kwargs or {})):
        if not mlp_plain and not nk.get("use_layer_norm", True):
            raise NotImplementedError(f"{which}: use_layer_norm=False ({served}{_PLAIN_HINT})")
        dims = nk.get("hidden_dims", [256, 256])
        dims = list(dims) if isinstance(dims, (list, tuple, np.ndarray)) else [dims]
        if not 1 <= len(dims) <= MAX_MLP_LAYERS:
            raise NotImplementedError(f"{which}: hidden_dims={dims} has {len(dims)} layers ({served})")
        for d in dims:
            if not _is_width(d):
                raise NotImplementedError(f"{which}: width {d!r} in hidden_dims={dims} is no integer ({served})")
            if int(d) not in (RAGGED_WIDTHS if mlp_ragged else HIDDEN_WIDTHS):
                raise NotImplementedError(f"{which}: width {int(d)} in hidden_dims={dims} is "
                                          f"{'outside [1, 1024]' if mlp_ragged else 'off the grid'} ({served})")
        out.append(tuple(int(d) for d in dims))
    return tuple(out)


def resolve_mlp_dims(hidden=256, critic_dims=None, policy_dims=None):
    """(critic, policy) width tuples from the defaulted parameters every shape helper takes: None means (hidden, hidden)."""
    return (tuple(int(d) for d in critic_dims) if critic_dims is not None else (int(hidden), int(hidden)),
            tuple(int(d) for d in policy_dims) if policy_dims is not None else (int(hidden), int(hidden)))


def _mlp_shapes(net, lead, fan_in, dims, layer_norm=True):
    """{leaf: shape} of one MLP, layer by layer as the arena lays them out; lead: () or (ensemble,).  layer_norm False
    (mlp.py:29-30, use_layer_norm=False): the kernels and biases alone."""
    sh = {}
    for j, d in enumerate(dims, 1):
        sh[f"{net}/w{j}"] = (*lead, fan_in, d)
        sh[f"{net}/b{j}"] = (*lead, d)
        if layer_norm:
            sh[f"{net}/ln{j}/scale"] = (*lead, d)
            sh[f"{net}/ln{j}/bias"] = (*lead, d)
        fan_in = d
    return sh


MLP_ACTIVATIONS = ("tanh", "relu", "swish")   # serl_agent_create_mlp's critic_act / policy_act (SERL_ACT_*), in code order
_ACTIVATION_NAMES = {"tanh": "tanh", "relu": "relu", "swish": "swish", "silu": "swish"}   # flax.linen.silu is swish


def mlp_activations(critic_network_kwargs=None, policy_network_kwargs=None, mlp_dropout=False):
    """(critic, policy): the `activations` of the reference's MLP (networks/mlp.py:19-31) from its two network kwargs, each one
    of MLP_ACTIVATIONS.  Accepted: the strings "tanh", "relu", "swish", "silu" (mlp.py resolves a string as getattr(nn, name)) and
    any callable whose __name__ is one of them (nn.tanh, jax.nn.relu, ...).  An absent key means what utils/launcher.py writes,
    tanh -- not mlp.py's own default, swish: pass it to get it.  Anything else, and a positive dropout_rate, raises
    NotImplementedError from the arguments alone -- unless the caller has switched MLP Dropout on (mlp_dropout=True, the
    argument of the same name of create_states / create_drq): the rates are then mlp_dropout_rates' to read and to refuse."""
    served = 'served: activations "tanh", "relu", "swish" (= "silu") by name or as a callable of that __name__, dropout_rate None or 0'
    out = []
    for which, nk in (("critic_network_kwargs", critic_network_kwargs or {}), ("policy_network_kwargs", policy_network_kwargs or {})):
        act = nk.get("activations", "tanh")
        name = act if isinstance(act, str) else getattr(act, "__name__", None) if callable(act) else None
        if not isinstance(name, str) or name not in _ACTIVATION_NAMES:
            raise NotImplementedError(f"{which}: activations={act!r} ({served})")
        rate = nk.get("dropout_rate")
        if not mlp_dropout and rate is not None and not (isinstance(rate, (int, float)) and rate <= 0):
            raise NotImplementedError(f"{which}: dropout_rate={rate!r} ({served}; a positive rate below 1 with mlp_dropout=True)")
        out.append(_ACTIVATION_NAMES[name])
    return tuple(out)


def mlp_layer_norms(critic_network_kwargs=None, policy_network_kwargs=None):
    """What create_states / create_drq read with mlp_plain=True (without it use_layer_norm=False is refused by mlp_hidden_width /
    mlp_layer_dims, as it always was).  (critic, policy): the `use_layer_norm` of the reference's MLP (networks/mlp.py:29-30) from its
    two network kwargs, as bools: serl_agent_create_layer_norm's two flags.  An absent key means what utils/launcher.py writes and
    this library has always meant, True -- not mlp.py's own default, False: pass it to get it.  Anything that is not a bool raises
    NotImplementedError from the arguments alone."""
    out = []
    for which, nk in (("critic_network_kwargs", critic_network_kwargs or {}), ("policy_network_kwargs", policy_network_kwargs or {})):
        flag = nk.get("use_layer_norm", True)
        if not isinstance(flag, (bool, np.bool_)):
            raise NotImplementedError(f"{which}: use_layer_norm={flag!r} (served: True or False)")
        out.append(bool(flag))
    return tuple(out)


def _dropout_rate_ok(rate):
    return rate is None or (not isinstance(rate, bool) and isinstance(rate, (int, float, np.integer, np.floating)) and bool(rate < 1))


def mlp_dropout_rates(critic_network_kwargs=None, policy_network_kwargs=None):
    """What create_states / create_drq read with mlp_dropout=True (without it a positive rate is refused by mlp_activations, as it
    always was).  (critic, policy): the `dropout_rate` of the reference's MLP (networks/mlp.py:27-28: Dense -> Dropout -> LayerNorm ->
    activation in both hidden layers) from its two network kwargs, as floats: serl_agent_create_dropout's two rates.  None, an
    absent key and anything <= 0 mean 0, as mlp.py reads them (`dropout_rate is not None and dropout_rate > 0`).  A rate >= 1 or
    a value that is no number raises NotImplementedError from the arguments alone."""
    served = "served: dropout_rate None or a number below 1 (<= 0 means no Dropout)"
    out = []
    for which, nk in (("critic_network_kwargs", critic_network_kwargs or {}), ("policy_network_kwargs", policy_network_kwargs or {})):
        rate = nk.get("dropout_rate")
        if rate is None:
            out.append(0.0)
            continue
        if not _dropout_rate_ok(rate):
            raise NotImplementedError(f"{which}: dropout_rate={rate!r} ({served})")
        out.append(max(float(rate), 0.0))
    return tuple(out)


STD_PARAMETERIZATIONS = ("exp", "softplus", "uniform")   # serl_agent_create_policy's std_param (actor_critic_nets.py:196-211); "fixed" is not served


def policy_mode(policy_kwargs=None):
    """(std_parameterization, tanh_squash_distribution) of the reference's `policy_kwargs`.  An absent key means what
    utils/launcher.py writes down ("exp", True), as it always did here -- also for policy_kwargs=None, where create_drq's own
    default dict would say "uniform": pass it to get it.  Anything the head kernels do not serve raises NotImplementedError."""
    pk = policy_kwargs or {}
    std = pk.get("std_parameterization", "exp")
    if std not in STD_PARAMETERIZATIONS:
        raise NotImplementedError(f"std_parameterization={std!r}: served are {STD_PARAMETERIZATIONS} (no 'fixed' / fixed_std)")
    if pk.get("fixed_std") is not None:
        raise NotImplementedError("policy_kwargs['fixed_std'] is not served")
    return std, bool(pk.get("tanh_squash_distribution", True))


FIXED_STD = "fixed"   # SERL_STD_FIXED: read by policy_mode_fixed alone (policy_fixed=True)


def policy_mode_fixed(policy_kwargs, A):
    """What create_states / create_drq read with policy_fixed=True (without it policy_mode reads and refuses as it always did).
    (std_parameterization, tanh_squash_distribution, fixed): std is "exp", "softplus", "uniform" or "fixed"; fixed is None, or
    with "fixed" a float32 vector of A entries -- `fixed_std`, a scalar (how sac.py's docstring writes TD3: fixed_std=0.1)
    broadcast to A or a sequence of A numbers.  The reference (actor_critic_nets.py:189-192,212-215) then builds neither Dense_1
    nor log_stds and uses stds = clip(fixed_std, std_min, std_max).  Refused from the arguments alone: fixed_std beside another
    std_parameterization (the reference asserts), "fixed" without fixed_std (ValueError, the reference's own "Invalid
    std_parameterization"), a length other than 1 or A, an entry that is not a finite positive number."""
    pk = policy_kwargs or {}
    std = pk.get("std_parameterization", "exp")
    fixed = pk.get("fixed_std")
    if std != FIXED_STD:
        if fixed is not None:
            raise NotImplementedError(f"policy_kwargs['fixed_std'] with std_parameterization={std!r}: fixed_std goes with "
                                      "std_parameterization='fixed' alone (actor_critic_nets.py:191 asserts it)")
        return (*policy_mode(pk), None)
    if fixed is None:
        raise ValueError("Invalid std_parameterization: 'fixed' without policy_kwargs['fixed_std'] (actor_critic_nets.py:209-210)")
    try:
        v = np.asarray(fixed, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"policy_kwargs['fixed_std']={fixed!r} is not a number or a sequence of {A} numbers") from None
    if v.ndim > 1 or v.size not in (1, A):
        raise ValueError(f"policy_kwargs['fixed_std'] has shape {v.shape}: served are a scalar and a vector of action_dim = {A} entries")
    with np.errstate(over="ignore"):     # (a double past float32's range becomes inf, and is refused below)
        v = np.broadcast_to(v.reshape(-1), (A,)).astype(np.float32)
    if not (np.isfinite(v).all() and (v > 0).all()):
        raise ValueError(f"policy_kwargs['fixed_std']={fixed!r}: every entry must be a finite positive number (as float32: {v.tolist()})")
    return FIXED_STD, bool(pk.get("tanh_squash_distribution", True)), v.copy()


@dataclasses.dataclass(frozen=True)
class NetSpec:
    """The options of an agent's critic and policy networks, stated once: what network_spec reads from the reference's kwargs, what
    AgentCore takes as keywords and hands to serl_agent_create_opts (to_c), and what the leaf tables are built from (leaf_kwargs).
    The defaults are what utils/launcher.py configures, and the all-zero serl_agent_opts.
    critic_dims / policy_dims: None means (hidden, hidden); with both None the library is sent n_layers = 0, "two layers of
    cfg.hidden", the agent every call without mlp_shapes makes.  fixed_std: None, or with "fixed" act_dim float32 values as floats.
    ragged: serl_agent_opts.ragged_widths -- the widths are any integers in [1, 1024]; network_spec sets it where a width is off the
    64 grid and nowhere else, so that widths on the grid through mlp_ragged=True give the NetSpec, and the agent, of the call without.
    use_proprio: False is serl_agent_opts.no_proprio -- EncodingWrapper(use_proprio=False) (common/encoding.py:53-72), the image codes
    alone: no enc/proprio/* leaf, and the first kernels of both MLPs lose the 64 proprio rows.  network_spec sets it from
    create_drq's use_proprio under image_only=True and nowhere else."""
    std_parameterization: str = "exp"
    tanh_squash_distribution: bool = True
    fixed_std: Optional[Tuple[float, ...]] = None
    critic_activation: str = "tanh"
    policy_activation: str = "tanh"
    critic_dropout: float = 0.0
    policy_dropout: float = 0.0
    hidden: int = 256
    critic_dims: Optional[Tuple[int, ...]] = None
    policy_dims: Optional[Tuple[int, ...]] = None
    critic_layer_norm: bool = True
    policy_layer_norm: bool = True
    ragged: bool = False
    use_proprio: bool = True

    @property
    def dims(self):
        """(critic, policy) width tuples, a list left out resolved"""
        return resolve_mlp_dims(self.hidden, self.critic_dims, self.policy_dims)

    @property
    def off_grid(self):
        """whether a width of either network is no multiple of 64"""
        return any(d % 64 for net in self.dims for d in net)

    def check(self):
        """A positive dropout_rate (mlp_dropout=True) is served in two LayerNorm MLPs of one [h, h] under a policy head with std
        leaves: the Dropout masks and per-layer keys of serl_mlp_noise are laid out for two layers of one width, the LayerNorm-free
        rows carry no Dropout, and the library serves none beside a fixed std.  Anything else raises NotImplementedError."""
        rates = (self.critic_dropout, self.policy_dropout)
        if not any(r > 0 for r in rates):
            return self
        if not self.use_proprio:
            raise NotImplementedError(
                f"use_proprio=False under image_only=True with mlp_dropout=True and a positive dropout_rate (critic {rates[0]!r} / policy "
                f"{rates[1]!r}) (served: Dropout in the MLPs of agents with the proprio branch)")
        cd, pd = self.dims
        if self.ragged and self.off_grid:
            raise NotImplementedError(
                f"mlp_ragged=True with mlp_dropout=True and a positive dropout_rate (critic {rates[0]!r} / policy {rates[1]!r}): critic "
                f"hidden_dims={list(cd)}, policy hidden_dims={list(pd)} (served with Dropout: widths that are multiples of 64; the "
                "keep-masks are laid out for rows of such a width)")
        if not (len(cd) == 2 and cd[0] == cd[1] and cd == pd):
            raise NotImplementedError(
                f"mlp_shapes=True with mlp_dropout=True and a positive dropout_rate: critic hidden_dims={list(cd)}, policy "
                f"hidden_dims={list(pd)} (served with Dropout: hidden_dims=[h, h], the same in both networks)")
        nets = (("critic_network_kwargs", self.critic_layer_norm, rates[0]), ("policy_network_kwargs", self.policy_layer_norm, rates[1]))
        for which, ln, rate in nets:
            if not ln and rate > 0:
                raise NotImplementedError(f"{which}: use_layer_norm=False under mlp_plain=True with dropout_rate={rate!r} under "
                                          "mlp_dropout=True (served: Dropout in agents whose two networks have their LayerNorm)")
        if not (self.critic_layer_norm and self.policy_layer_norm):
            which, _, rate = next(n for n in nets if n[2] > 0)
            raise NotImplementedError(f"{which}: dropout_rate={rate!r} under mlp_dropout=True beside a network with use_layer_norm=False "
                                      "under mlp_plain=True (served: Dropout in agents whose two networks have their LayerNorm)")
        if self.fixed_std is not None:
            raise NotImplementedError(f"std_parameterization='fixed' under policy_fixed=True with dropout_rate critic {rates[0]!r} / "
                                      f"policy {rates[1]!r} under mlp_dropout=True (served: Dropout in agents whose policy head has std leaves)")
        return self

    def core_kwargs(self):
        """AgentCore's keywords of these options"""
        return dataclasses.asdict(self)

    def leaf_kwargs(self):
        """what the leaf tables depend on, as theta_shapes, init_theta, flax_tree.theta_paths and init_ref.theta_leaves /
        theta_reference all take it"""
        cd, pd = self.dims
        return dict(std_parameterization=self.std_parameterization, critic_dims=cd, policy_dims=pd,
                    critic_layer_norm=self.critic_layer_norm, policy_layer_norm=self.policy_layer_norm,
                    **({} if self.use_proprio else {"use_proprio": False}))

    def config_entries(self):
        """the network entries of agent.config; fixed_std, the use_layer_norm pair and use_proprio (False: the image-only agent)
        only where they say something"""
        return dict(**({} if self.use_proprio else {"use_proprio": False}),
                    critic_activation=self.critic_activation, policy_activation=self.policy_activation,
                    critic_dropout_rate=self.critic_dropout, policy_dropout_rate=self.policy_dropout,
                    **({} if self.fixed_std is None else {"fixed_std": self.fixed_std}),
                    **({} if self.critic_layer_norm and self.policy_layer_norm else
                       {"critic_use_layer_norm": self.critic_layer_norm, "policy_use_layer_norm": self.policy_layer_norm}))

    def to_c(self):
        """-> _lib_agent.SerlAgentOpts (serl_agent_opts); no device is touched.  (ctypes keeps the fixed_std buffer alive with the struct.)"""
        from .._lib_agent import SerlAgentOpts
        o = SerlAgentOpts()
        o.std_param = 3 if self.fixed_std is not None else STD_PARAMETERIZATIONS.index(self.std_parameterization)   # SERL_STD_FIXED = 3
        o.no_tanh = 0 if self.tanh_squash_distribution else 1
        given = self.critic_dims is not None or self.policy_dims is not None
        for net, act, dims, ln, rate in zip((o.critic, o.policy), (self.critic_activation, self.policy_activation), self.dims,
                                            (self.critic_layer_norm, self.policy_layer_norm), (self.critic_dropout, self.policy_dropout)):
            net.act = MLP_ACTIVATIONS.index(act)
            if given:
                net.n_layers, net.dims[:len(dims)] = len(dims), dims
            net.no_layer_norm, net.dropout = 0 if ln else 1, rate
        if self.fixed_std is not None:
            o.fixed_std = (ctypes.c_float * len(self.fixed_std))(*self.fixed_std)
        o.ragged_widths = 1 if self.ragged else 0
        o.no_proprio = 0 if self.use_proprio else 1
        return o


def network_spec(critic_network_kwargs, policy_network_kwargs, policy_kwargs, act_dim, *, mlp_dropout=False, mlp_shapes=False,
                 mlp_plain=False, policy_fixed=False, mlp_ragged=False, use_proprio=True) -> NetSpec:
    """The checked NetSpec of create_states' / create_drq's three kwargs dicts under their five switches; every refusal is raised
    from the arguments alone, in the order of the lines below.  mlp_ragged=True: every width read below is any integer in
    [1, 1024] (mlp.py:19-31 takes any list); without it the 64 grid, as always.  use_proprio: create_drq's, already checked to be
    a bool and read under image_only=True alone."""
    # policy_fixed=True: "fixed" / fixed_std are read (actor_critic_nets.py:189-192); else refused, as always
    std_param, squash, fixed = policy_mode_fixed(policy_kwargs, act_dim) if policy_fixed else (*policy_mode(policy_kwargs), None)
    # mlp_shapes=True: each network's own depth and per-layer widths (mlp.py:19-31); else the one width of [h, h], as always
    dims = mlp_layer_dims(critic_network_kwargs, policy_network_kwargs, mlp_plain, mlp_ragged) if mlp_shapes else (None, None)
    hidden = dims[0][0] if mlp_shapes else mlp_hidden_width(critic_network_kwargs, policy_network_kwargs, mlp_plain, mlp_ragged)
    # mlp_plain=True: each network's own use_layer_norm (mlp.py:29-30); else LayerNorm in both, as always
    lns = mlp_layer_norms(critic_network_kwargs, policy_network_kwargs) if mlp_plain else (True, True)
    acts = mlp_activations(critic_network_kwargs, policy_network_kwargs, mlp_dropout)
    rates = mlp_dropout_rates(critic_network_kwargs, policy_network_kwargs) if mlp_dropout else (0.0, 0.0)
    if dims == ((hidden, hidden), (hidden, hidden)):
        dims = (None, None)    # [h, h] twice: the very agent the call without the switch makes
    spec = NetSpec(std_param, squash, None if fixed is None else tuple(float(x) for x in fixed), *acts, *rates, hidden, *dims, *lns)
    return dataclasses.replace(spec, ragged=bool(mlp_ragged) and spec.off_grid, use_proprio=bool(use_proprio)).check()


def _policy_std_shapes(Hd, A, std_parameterization):
    """The leaves behind the policy's mean head: Dense_1 (log-std or softplus pre-activation), or with "uniform" the one
    `log_stds` vector shared by all rows (actor_critic_nets.py:199-201); none with "fixed" (:190-192: no std parameter)."""
    if std_parameterization == FIXED_STD:
        return {}
    if std_parameterization not in STD_PARAMETERIZATIONS:
        raise NotImplementedError(f"std_parameterization={std_parameterization!r}")
    if std_parameterization == "uniform":
        return {"actor/log_stds": (A,)}
    return {"actor/logstd/kernel": (Hd, A), "actor/logstd/bias": (A,)}


def theta_shapes(n_cam, H, W, S, A, ensemble=10, hidden=256, bottleneck=256, sle_features=8, proprio_dim=64,
                 encoder_type="resnet-pretrained", num_stack=1, std_parameterization="exp", critic_dims=None, policy_dims=None, critic_layer_norm=True,
                 policy_layer_norm=True, use_proprio=True):
    """use_proprio False (pixel agents): no enc/proprio/* leaf, and E = bottleneck * n_cam.
    critic_dims / policy_dims: the hidden widths of each MLP, layer by layer (None: (hidden, hidden)); the heads follow the last.
    critic_layer_norm / policy_layer_norm False: that MLP's layers own w<j> and b<j> alone (mlp.py:29-30, use_layer_norm=False).
    S: the proprio Dense's input width -- T * S for a stack of T = num_stack frames, which EncodingWrapper folds into the
    channels ("B T H W C -> B H W (T C)", common/encoding.py:39-44): the SmallEncoder's first kernel is then (3,3,3T,32).
    std_parameterization="uniform": actor/log_stds (A,) in place of actor/logstd/{kernel,bias}; "fixed": neither."""
    cd, pd = resolve_mlp_dims(hidden, critic_dims, policy_dims)
    if n_cam == 0:   # state-only SAC (SACAgent.create_states, sac.py:486-542): no encoder, per-member Q heads
        N = ensemble
        return {
            **_mlp_shapes("critic", (N,), S + A, cd, critic_layer_norm),
            "critic/head/kernel": (N, cd[-1], 1), "critic/head/bias": (N, 1),   # vmapped Dense(1): one bias per member
            **_mlp_shapes("actor", (), S, pd, policy_layer_norm),
            "actor/mean/kernel": (pd[-1], A), "actor/mean/bias": (A,),
            **_policy_std_shapes(pd[-1], A, std_parameterization),
            "temp/lagrange": (),
        }
    fh, fw = feat_hw(H, W)
    E = bottleneck * n_cam + (proprio_dim if use_proprio else 0)
    sh = {}
    for k in range(n_cam):
        if encoder_type == "small":    # 4 x Conv(3x3, stride 2, VALID) with bias, then mean-pool -> Dense(256)
            for l in range(4):
                sh[f"enc/{k}/conv{l}/kernel"] = (3, 3, SMALL_FEATURES[l] * (num_stack if l == 0 else 1), SMALL_FEATURES[l + 1])
                sh[f"enc/{k}/conv{l}/bias"] = (SMALL_FEATURES[l + 1],)
            sh[f"enc/{k}/dense/kernel"] = (SMALL_FEATURES[4], bottleneck)
        else:
            sh[f"enc/{k}/sle"] = (fh, fw, 512, sle_features)
            sh[f"enc/{k}/dense/kernel"] = (512 * sle_features, bottleneck)
        sh[f"enc/{k}/dense/bias"] = (bottleneck,)
        sh[f"enc/{k}/ln/scale"] = (bottleneck,)
        sh[f"enc/{k}/ln/bias"] = (bottleneck,)
    N = ensemble
    sh.update({
        **_mlp_shapes("critic", (N,), E + A, cd, critic_layer_norm),
        "critic/head/kernel": (cd[-1], 1), "critic/head/bias": (1,),
        **({"enc/proprio/dense/kernel": (S, proprio_dim), "enc/proprio/dense/bias": (proprio_dim,),
            "enc/proprio/ln/scale": (proprio_dim,), "enc/proprio/ln/bias": (proprio_dim,)} if use_proprio else {}),
        **_mlp_shapes("actor", (), E, pd, policy_layer_norm),
        "actor/mean/kernel": (pd[-1], A), "actor/mean/bias": (A,),
        **_policy_std_shapes(pd[-1], A, std_parameterization),
        "temp/lagrange": (),
    })
    return sh


_MLP_KERNEL = re.compile(r"(critic|actor)/w[1-9]")     # the Dense kernels of the two MLPs


def init_trunk(seed=42):
    rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([seed, 1])))
    out = {}
    for name, shp in trunk_shapes().items():
        if len(shp) == 4:  # nn.initializers.kaiming_normal (resnet_v1.py:228-233)
            out[name] = (rng.standard_normal(shp) * math.sqrt(2.0 / (shp[0] * shp[1] * shp[2]))).astype(np.float32)
        elif name.endswith("scale"):
            out[name] = np.ones(shp, np.float32)
        else:
            out[name] = np.zeros(shp, np.float32)
    return out


def init_theta(n_cam, H, W, S, A, seed=42, temperature_init=1e-2, **kw):
    if not kw.get("use_proprio", True) and n_cam > 0:
        # The image-only agent: the draw of the proprio agent of the same seed, so that every leaf the two share keeps its values;
        # enc/proprio/* is dropped, and the two first kernels lose the rows of the 64 proprio columns (the last of the code) and
        # are rescaled to the xavier-uniform bound of their new fan-in.
        full = init_theta(n_cam, H, W, S, A, seed=seed, temperature_init=temperature_init, **{**kw, "use_proprio": True})
        out = {}
        Eimg = kw.get("bottleneck", 256) * n_cam      # the code's width; the proprio columns were [Eimg, Eimg + proprio_dim)
        Efull = Eimg + kw.get("proprio_dim", 64)
        for name, shp in theta_shapes(n_cam, H, W, S, A, **kw).items():
            v = full[name]
            if name in ("critic/w1", "actor/w1"):     # (N, E + A, d) and (E, d): the rows [Eimg, Efull) leave
                keep = np.r_[0:Eimg, Efull:v.shape[-2]]
                scale = math.sqrt((v.shape[-2] + v.shape[-1]) / (shp[-2] + shp[-1]))
                v = (np.take(v, keep, axis=-2).astype(np.float64) * scale).astype(np.float32)
            assert v.shape == tuple(shp), (name, v.shape, shp)
            out[name] = v
        return out
    rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([seed, 2])))
    out = {}
    for name, shp in theta_shapes(n_cam, H, W, S, A, **kw).items():
        if name.endswith("/sle"):  # lecun_normal over (h,w,c) (resnet_v1.py:86)
            out[name] = (rng.standard_normal(shp) / math.sqrt(shp[0] * shp[1] * shp[2])).astype(np.float32)
        elif name.startswith("enc/") and "/conv" in name and name.endswith("kernel"):   # nn.Conv default lecun_normal
            out[name] = (rng.standard_normal(shp) / math.sqrt(shp[0] * shp[1] * shp[2])).astype(np.float32)
        elif name.startswith("enc/") and name.endswith("dense/kernel") and "proprio" not in name:
            out[name] = (rng.standard_normal(shp) / math.sqrt(shp[0])).astype(np.float32)  # nn.Dense default
        elif _MLP_KERNEL.fullmatch(name) and name.startswith("critic/") or (name == "critic/head/kernel" and len(shp) == 3):
            # default_init = xavier_uniform, vmapped per member
            a = math.sqrt(6.0 / (shp[1] + shp[2]))
            out[name] = rng.uniform(-a, a, shp).astype(np.float32)
        elif name.endswith("kernel") or _MLP_KERNEL.fullmatch(name):
            a = math.sqrt(6.0 / (shp[0] + shp[1]))
            out[name] = rng.uniform(-a, a, shp).astype(np.float32)
        elif name.endswith("scale"):
            out[name] = np.ones(shp, np.float32)
        elif name == "temp/lagrange":  # lagrange.py:28-29
            out[name] = np.float32(math.log(math.exp(temperature_init) - 1.0))
        else:
            out[name] = np.zeros(shp, np.float32)
    return out


def init_classifier(n_cam, H, W, seed=42):
    """Initial parameters of the reward classifier's trainable part (networks/reward_classifier.py:16-28 over
    EncodingWrapper(use_proprio=False)): camera heads as in init_theta (SpatialLearnedEmbeddings lecun-normal, Dense
    xavier-uniform, LayerNorm ones/zeros -- resnet_v1.py:94-104,363-374), Dense layers of the head with flax's default
    lecun-normal kernels and zero biases.  Host-side numpy streams, not jax's threefry (as for the agents)."""
    theta = init_theta(n_cam, H, W, 4, 2, seed=seed)
    out = {k: v for k, v in theta.items() if k.startswith("enc/") and not k.startswith("enc/proprio")}
    rng = np.random.default_rng(seed + 77)
    E = 256 * n_cam

    def lecun(fan_in, shape):   # jax.nn.initializers.lecun_normal: truncated normal, std = sqrt(1 / fan_in) / 0.8796
        std = math.sqrt(1.0 / fan_in) / 0.87962566103423978
        v = rng.standard_normal(shape)
        bad = np.abs(v) > 2.0
        while bad.any():
            v[bad] = rng.standard_normal(int(bad.sum()))
            bad = np.abs(v) > 2.0
        return (v * std).astype(np.float32)
    out["head/dense0/kernel"] = lecun(E, (E, 256))
    out["head/dense0/bias"] = np.zeros(256, np.float32)
    out["head/ln/scale"] = np.ones(256, np.float32)
    out["head/ln/bias"] = np.zeros(256, np.float32)
    out["head/dense1/kernel"] = lecun(256, (256, 1))
    out["head/dense1/bias"] = np.zeros(1, np.float32)
    return out
