"""CPU: an agent's network options stated once -- utils.init.NetSpec on the Python side, serl_agent_opts in the C ABI
(include/serl_mi355.h, NETWORK OPTIONS).

* the ctypes mirror of serl_agent_opts against the library, field by field: serl_agent_create_opts returns its argument errors
  before any device call, and each message names the field that was wrong and its value;
* the three combinations the struct can state and the older argument lists could not are refused by the library;
* NetSpec.to_c() over a table of specs;
* create_states and create_drq read the same kwargs into the same NetSpec, and refuse the same kwargs in the same words."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import mlp_plain as MP
import mlp_shapes as MS
import mlp_widths as MW
import policy_modes as PM
from serl_amd.utils import init as pinit
from serl_amd.utils.init import NetSpec
from test_mlp_activations_cpu import BAD
from test_mlp_shapes_cpu import SHAPE_REFUSALS
from test_mlp_widths_cpu import REFUSALS

SERL_ERR_INVALID = -1      # include/serl_mi355.h
S, A = 10, 4


def _cfg(hidden=64):
    from serl_amd._lib_agent import SerlAgentCfg
    # state-only: n_cam 0, state_dim S, act_dim A, batch 8, ensemble 2
    return SerlAgentCfg(0, 0, 0, 0, S, A, 8, 2, hidden, 256, 8, 64, 0, -1, 0.99, 0.005, 3e-4, 0.1, 1e-5, 5.0, -2.0, 0)


def _create(opts, cfg=None):
    """serl_agent_create_opts -> (status, serl_last_error()); an agent that was made (a device is present) is destroyed again"""
    from serl_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    rc = int(L.serl_agent_create_opts(C.byref(cfg or _cfg()), C.byref(opts), C.byref(h)))
    msg = (L.serl_last_error() or b"").decode()
    if rc == 0:
        assert int(L.serl_agent_destroy(h)) == 0
    return rc, msg


def _valid():
    """an options struct that uses every field and is valid: four layers per network, no LayerNorm in the policy, a fixed std"""
    from serl_amd._lib_agent import SerlAgentOpts
    o = SerlAgentOpts()
    o.std_param, o.no_tanh = 3, 1
    o.critic.act, o.critic.n_layers, o.critic.dims[:] = 2, 4, (64, 128, 192, 256)
    o.policy.act, o.policy.n_layers, o.policy.dims[:], o.policy.no_layer_norm = 1, 4, (320, 384, 448, 512), 1
    o.fixed_std = (C.c_float * A)(0.1, 0.2, 0.3, 0.4)
    return o


def _set(path, value):
    def apply(o):
        *owners, name = path.split(".")
        for k in owners:
            o = getattr(o, k)
        if "[" in name:
            name, j = name[:-1].split("[")
            getattr(o, name)[int(j)] = value
        else:
            setattr(o, name, value)
    return apply


# field (as the ctypes mirror names it) -> a value the library refuses, what its message says
FIELDS = [
    ("std_param", 7, "std_param 7 is not"),
    ("no_tanh", 2, "no_tanh 2 is not"),
    ("critic.act", 7, "critic_act 7:"),
    ("critic.n_layers", 5, "critic MLP: 5 hidden layers"),
    *[(f"critic.dims[{j}]", 100, f"critic MLP: layer {j + 1} has width 100") for j in range(4)],
    ("critic.no_layer_norm", 2, "critic no_layer_norm 2 is not"),
    ("critic.dropout", 1.5, "critic_dropout 1.5:"),
    ("policy.act", -1, "policy_act -1:"),
    ("policy.n_layers", -2, "policy MLP: -2 hidden layers"),
    *[(f"policy.dims[{j}]", 1088, f"policy MLP: layer {j + 1} has width 1088") for j in range(4)],
    ("policy.no_layer_norm", -1, "policy no_layer_norm -1 is not"),
    ("policy.dropout", -0.25, "policy_dropout -0.25:"),
]


def test_the_valid_struct_is_not_refused_for_its_arguments():
    """(without a device the call ends at hipSetDevice, with one it makes the agent: either way no argument error)"""
    rc, msg = _create(_valid())
    assert rc != SERL_ERR_INVALID, (rc, msg)


@pytest.mark.parametrize("path,value,what", FIELDS, ids=[f[0] for f in FIELDS])
def test_each_field_of_the_mirror_is_the_field_the_library_reads(path, value, what):
    o = _valid()
    _set(path, value)(o)
    rc, msg = _create(o)
    assert rc == SERL_ERR_INVALID and what in msg, (path, rc, msg)


def test_fixed_std_pointer_is_the_last_field():
    o = _valid()
    o.fixed_std = (C.c_float * A)(0.1, 0.0, 0.3, 0.4)
    rc, msg = _create(o)
    assert rc == SERL_ERR_INVALID and "fixed_std[1] = 0" in msg, (rc, msg)
    o = _valid()
    o.fixed_std = None
    rc, msg = _create(o)
    assert rc == SERL_ERR_INVALID and "needs fixed_std" in msg, (rc, msg)
    o = _valid()
    o.std_param = 0
    rc, msg = _create(o)
    assert rc == SERL_ERR_INVALID and "fixed_std is given with std_param 0" in msg, (rc, msg)


def test_zero_layers_means_cfg_hidden_and_is_checked_as_hidden():
    from serl_amd._lib_agent import SerlAgentOpts
    rc, msg = _create(SerlAgentOpts(), _cfg(hidden=100))
    assert rc == SERL_ERR_INVALID and "hidden must be a multiple of 64 in [64, 1024] (got 100)" in msg, (rc, msg)
    o = SerlAgentOpts()      # one network with its own list: cfg.hidden still stands for the other
    o.policy.n_layers, o.policy.dims[0] = 1, 64
    rc, msg = _create(o, _cfg(hidden=100))
    assert rc == SERL_ERR_INVALID and "hidden must be a multiple of 64" in msg, (rc, msg)
    o.critic.n_layers, o.critic.dims[0] = 1, 128      # both lists given: cfg.hidden is not read
    rc, msg = _create(o, _cfg(hidden=100))
    assert rc != SERL_ERR_INVALID, (rc, msg)
    rc, msg = _create(SerlAgentOpts())      # all zero: serl_agent_create(cfg)
    assert rc != SERL_ERR_INVALID, (rc, msg)


def test_a_zero_count_through_an_older_entry_point_is_refused_as_zero_layers():
    """serl_agent_create_shapes / _layer_norm / _fixed_std: a caller's 0 never becomes "use cfg->hidden", and a count past the
    array is refused before anything is copied"""
    from serl_amd import _lib
    L, cfg, h = _lib.lib(), _cfg(), C.c_void_p()
    dims = (C.c_int32 * 4)(64, 64, 64, 64)
    for n_critic, n_policy, what in ((0, 2, "critic MLP: 0 hidden layers"), (2, 0, "policy MLP: 0 hidden layers"),
                                     (9, 2, "critic MLP: 9 hidden layers"), (1, 1 << 20, f"policy MLP: {1 << 20} hidden layers")):
        for rc in (int(L.serl_agent_create_shapes(C.byref(cfg), 0, 0, 0, 0, dims, n_critic, dims, n_policy, C.byref(h))),
                   int(L.serl_agent_create_layer_norm(C.byref(cfg), 0, 0, 0, 0, dims, n_critic, dims, n_policy, 1, 1, C.byref(h))),
                   int(L.serl_agent_create_fixed_std(C.byref(cfg), 0, 0, 0, 0, dims, n_critic, dims, n_policy, 1, 1, None, C.byref(h)))):
            msg = (L.serl_last_error() or b"").decode()
            assert rc == SERL_ERR_INVALID and what in msg and "served: 1 to 4 layers" in msg and not h.value, (n_critic, n_policy, rc, msg)


# ---- what the struct can say and the argument lists could not --------------------------------------------------------------------
def test_dropout_stays_where_it_was_served():
    from serl_amd._lib_agent import SerlAgentOpts
    for rates in ((0.1, 0.0), (0.0, 0.2)):
        def opts():
            o = SerlAgentOpts()
            o.critic.dropout, o.policy.dropout = rates
            return o
        rc, msg = _create(opts())
        assert rc != SERL_ERR_INVALID, (rc, msg)      # two layers of cfg.hidden, LayerNorm, std leaves: served
        o = opts()
        o.policy.n_layers, o.policy.dims[:2] = 2, (64, 64)
        rc, msg = _create(o)
        assert rc == SERL_ERR_INVALID and "n_layers 0 / 2" in msg and "dropout" in msg and "n_layers 0 in both networks" in msg, (rc, msg)
        for net in ("critic", "policy"):
            o = opts()
            getattr(o, net).no_layer_norm = 1
            rc, msg = _create(o)
            assert rc == SERL_ERR_INVALID and "dropout" in msg.lower() and "LayerNorm" in msg, (rc, msg)
        o = opts()      # a rate in the LayerNorm network beside a plain one: named by its fields
        (o.policy if rates[0] > 0 else o.critic).no_layer_norm = 1
        rc, msg = _create(o)
        assert rc == SERL_ERR_INVALID and "no_layer_norm" in msg and "two networks have their LayerNorm" in msg, (rc, msg)
        o = opts()
        o.std_param, o.fixed_std = 3, (C.c_float * A)(0.1, 0.2, 0.3, 0.4)
        rc, msg = _create(o)
        assert rc == SERL_ERR_INVALID and "with std_param SERL_STD_FIXED (3)" in msg and "dropout" in msg, (rc, msg)


# ---- NetSpec -> serl_agent_opts ------------------------------------------------------------------------------------------------------
def _fields(o):
    net = lambda m: (m.act, m.n_layers, tuple(m.dims), m.no_layer_norm, m.dropout)      # noqa: E731
    return (o.std_param, o.no_tanh, net(o.critic), net(o.policy), None if not o.fixed_std else tuple(o.fixed_std[j] for j in range(A)))


ZERO = (0, 0, (0, 0, 0, 0), 0, 0.0)
F32 = tuple(float(np.float32(x)) for x in (0.1, 0.2, 0.3, 0.4))
TO_C = [
    ("default", NetSpec(), (0, 0, ZERO, ZERO, None)),
    ("softplus", NetSpec(std_parameterization="softplus"), (1, 0, ZERO, ZERO, None)),
    ("uniform_gauss", NetSpec(std_parameterization="uniform", tanh_squash_distribution=False), (2, 1, ZERO, ZERO, None)),
    ("fixed", NetSpec(std_parameterization="fixed", fixed_std=F32), (3, 0, ZERO, ZERO, F32)),
    ("mixed_activations", NetSpec(critic_activation="swish", policy_activation="relu"), (0, 0, (2, *ZERO[1:]), (1, *ZERO[1:]), None)),
    ("critic_rate", NetSpec(critic_dropout=0.25, hidden=128), (0, 0, (*ZERO[:4], 0.25), ZERO, None)),
    ("one_list", NetSpec(policy_dims=(64, 128, 192), hidden=320), (0, 0, (0, 2, (320, 320, 0, 0), 0, 0.0), (0, 3, (64, 128, 192, 0), 0, 0.0), None)),
    ("h_h_twice", NetSpec(critic_dims=(128, 128), policy_dims=(128, 128), hidden=128),
     (0, 0, (0, 2, (128, 128, 0, 0), 0, 0.0), (0, 2, (128, 128, 0, 0), 0, 0.0), None)),
    ("plain_critic", NetSpec(critic_layer_norm=False), (0, 0, (0, 0, (0, 0, 0, 0), 1, 0.0), ZERO, None)),
    ("plain_policy", NetSpec(policy_layer_norm=False, critic_dims=(64,), policy_dims=(1024, 64, 64, 64)),
     (0, 0, (0, 1, (64, 0, 0, 0), 0, 0.0), (0, 4, (1024, 64, 64, 64), 1, 0.0), None)),
]


@pytest.mark.parametrize("spec,want", [r[1:] for r in TO_C], ids=[r[0] for r in TO_C])
def test_to_c_fills_the_struct(spec, want):
    assert _fields(spec.check().to_c()) == want
    assert spec.leaf_kwargs()["critic_dims"] == (spec.critic_dims or (spec.hidden, spec.hidden))


def test_to_c_refuses_names_the_library_has_no_code_for():
    for bad in (NetSpec(std_parameterization="tanh"), NetSpec(critic_activation="gelu")):
        with pytest.raises(ValueError):
            bad.to_c()


# ---- one parser for both constructors ------------------------------------------------------------------------------------------------
class _Stop(Exception):
    pass


def _spec_of(create, monkeypatch, **kw):
    """the NetSpec create_states / create_drq build from kw, or the exception they refuse kw with; no core is made"""
    import serl_amd.agents.drq as drq
    import serl_amd.agents.sac as sac
    from serl_amd.agents.drq import DrQAgent
    from serl_amd.agents.sac import SACAgent
    seen = []
    real = pinit.network_spec

    def network_spec(*a, **k):
        seen.append(real(*a, **k))
        return seen[-1]

    def no_core(**k):
        assert NetSpec(**{f.name: k[f.name] for f in dataclasses.fields(NetSpec) if f.name != "fixed_std"},
                       fixed_std=None if k["fixed_std"] is None else tuple(float(x) for x in k["fixed_std"])) == seen[-1]
        raise _Stop
    with monkeypatch.context() as m:
        m.setattr(pinit, "network_spec", network_spec)
        m.setattr(drq, "AgentCore", no_core)
        m.setattr(sac, "AgentCore", no_core)
        try:
            if create == "states":
                SACAgent.create_states(0, np.zeros((S,), np.float32), np.zeros((A,), np.float32), **kw)
            else:
                obs = {"image": np.zeros((1, 64, 64, 3), np.uint8), "state": np.zeros((1, 5), np.float32)}
                DrQAgent.create_drq(0, obs, np.zeros((A,), np.float32), encoder_type="resnet-pretrained", use_proprio=True,
                                    image_keys=("image",), **kw)
        except _Stop:
            return seen[-1]
        except (NotImplementedError, ValueError) as e:
            return type(e), str(e)
    raise AssertionError("a core was made")


_PK = dict(MW.POLICY_KWARGS)
ROWS = (
    [(f"widths_{r[0]}", dict(policy_kwargs=_PK, **r[1]), False) for r in REFUSALS]
    + [(f"shapes_{r[0]}", dict(policy_kwargs=_PK, mlp_shapes=True, **r[1]), False) for r in SHAPE_REFUSALS]
    + [(f"act_{b[0]}", dict(policy_kwargs=_PK, critic_network_kwargs={**MW.mlp_kwargs(128), **b[1]}, policy_network_kwargs=MW.mlp_kwargs(128)), False)
       for b in BAD[:3]]
    + [("dropout_other_shapes", dict(mlp_shapes=True, mlp_dropout=True, critic_network_kwargs=MS.mlp_kwargs([128, 256], dropout_rate=0.1),
                                     policy_network_kwargs=MS.mlp_kwargs([128, 256])), False),
       ("dropout_plain", dict(mlp_plain=True, mlp_dropout=True, critic_network_kwargs=MP.mlp_kwargs([128, 128], True, dropout_rate=0.1),
                              policy_network_kwargs=MP.mlp_kwargs([128, 128], False)), False),
       ("dropout_fixed", dict(policy_kwargs=dict(_PK, std_parameterization="fixed", fixed_std=0.1), policy_fixed=True, mlp_dropout=True,
                              critic_network_kwargs={"dropout_rate": 0.1}), False),
       ("fixed_without_the_switch", dict(policy_kwargs=dict(_PK, std_parameterization="fixed", fixed_std=0.1)), False),
       ("fixed_without_a_vector", dict(policy_kwargs=dict(_PK, std_parameterization="fixed"), policy_fixed=True), False),
       # served
       ("default", {}, True),
       ("launcher", dict(policy_kwargs=_PK, critic_network_kwargs=MW.mlp_kwargs(256), policy_network_kwargs=MW.mlp_kwargs(256)), True),
       ("width_128_swish_relu", dict(critic_network_kwargs=MW.mlp_kwargs(128, activations="swish"),
                                     policy_network_kwargs=MW.mlp_kwargs(128, activations="relu")), True),
       ("uniform_gauss", dict(policy_kwargs=PM.policy_kwargs("uniform", False)), True),
       ("shapes", dict(mlp_shapes=True, critic_network_kwargs=MS.mlp_kwargs([128, 256, 64]), policy_network_kwargs=MS.mlp_kwargs([64])), True),
       ("shapes_h_h_twice", dict(mlp_shapes=True, critic_network_kwargs=MS.mlp_kwargs([192, 192]), policy_network_kwargs=MS.mlp_kwargs([192, 192])), True),
       ("plain_policy", dict(mlp_plain=True, mlp_shapes=True, critic_network_kwargs=MP.mlp_kwargs([320], True),
                             policy_network_kwargs=MP.mlp_kwargs([64, 128], False)), True),
       ("dropout", dict(mlp_dropout=True, critic_network_kwargs=MW.mlp_kwargs(128, dropout_rate=0.1),
                        policy_network_kwargs=MW.mlp_kwargs(128, dropout_rate=0.25)), True),
       ("fixed_scalar", dict(policy_kwargs=dict(_PK, std_parameterization="fixed", fixed_std=0.1), policy_fixed=True), True)])


@pytest.mark.parametrize("kw,served", [r[1:] for r in ROWS], ids=[r[0] for r in ROWS])
def test_create_states_and_create_drq_read_the_same_spec(kw, served, monkeypatch):
    a, b = _spec_of("states", monkeypatch, **kw), _spec_of("drq", monkeypatch, **kw)
    assert a == b and isinstance(a, NetSpec) == served, (a, b)


def test_the_spec_of_a_call_is_what_its_kwargs_say(monkeypatch):
    spec = _spec_of("states", monkeypatch, **[r[1] for r in ROWS if r[0] == "plain_policy"][0])
    assert spec == NetSpec(hidden=320, critic_dims=(320,), policy_dims=(64, 128), policy_layer_norm=False)
    assert spec.config_entries() == dict(critic_activation="tanh", policy_activation="tanh", critic_dropout_rate=0.0, policy_dropout_rate=0.0,
                                         critic_use_layer_norm=True, policy_use_layer_norm=False)
    spec = _spec_of("drq", monkeypatch, **[r[1] for r in ROWS if r[0] == "shapes_h_h_twice"][0])
    assert spec == NetSpec(hidden=192) and _fields(spec.to_c()) == (0, 0, ZERO, ZERO, None)      # n_layers 0: the call without the switch
    assert set(spec.config_entries()) == {"critic_activation", "policy_activation", "critic_dropout_rate", "policy_dropout_rate"}
    spec = _spec_of("drq", monkeypatch, **[r[1] for r in ROWS if r[0] == "fixed_scalar"][0])
    assert spec.fixed_std == (float(np.float32(0.1)),) * A and spec.config_entries()["fixed_std"] == spec.fixed_std
