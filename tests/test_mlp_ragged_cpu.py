"""CPU: critic and policy MLP widths off the 64 grid (mlp_ragged=True, serl_agent_opts.ragged_widths): the refusals with and
without the switch on both sides of the C ABI, NetSpec.to_c(), the leaf tables and the flax tree at true shapes, the oracle at
(h, h) through the switch, and the relu condition of the GPU case table (tests/mlp_ragged.py).

Every test fails on a tree without the switch: network_spec, NetSpec and SerlAgentOpts do not know it."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import drq_oracle as O
import agent_helpers as AH
import mlp_ragged as MR
import mlp_shapes as MS
from serl_amd.utils import init as pinit
from serl_amd.utils.init import NetSpec
from test_agent_opts_cpu import SERL_ERR_INVALID, _cfg, _create

A = 4


def _kw(cd, pd, **extra):
    return dict(critic_network_kwargs=MS.mlp_kwargs(cd, **extra), policy_network_kwargs=MS.mlp_kwargs(pd))


# ---- Python: what the arguments alone decide ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [[400, 300], [100, 100], [50], [1], [1000, 3, 1024]])
def test_widths_off_the_grid_are_served_with_the_switch_and_refused_without(dims):
    with pytest.raises(NotImplementedError, match="is off the grid"):
        pinit.network_spec(*_kw(dims, dims).values(), None, A, mlp_shapes=True)
    spec = pinit.network_spec(*_kw(dims, [64]).values(), None, A, mlp_shapes=True, mlp_ragged=True)
    assert spec.ragged and spec.critic_dims == tuple(dims) and spec.policy_dims == (64,)
    assert spec.to_c().ragged_widths == 1 and tuple(spec.to_c().critic.dims[:len(dims)]) == tuple(dims)
    assert spec.core_kwargs()["ragged"] is True and spec.leaf_kwargs()["critic_dims"] == tuple(dims)


def test_one_width_for_both_networks_without_mlp_shapes():
    assert pinit.mlp_hidden_width(*_kw([100, 100], [100, 100]).values(), mlp_ragged=True) == 100
    spec = pinit.network_spec(*_kw([100, 100], [100, 100]).values(), None, A, mlp_ragged=True)
    assert spec == NetSpec(hidden=100, ragged=True) and spec.dims == ((100, 100), (100, 100))
    o = spec.to_c()
    assert (o.ragged_widths, o.critic.n_layers, o.policy.n_layers) == (1, 0, 0)      # two layers of cfg.hidden
    with pytest.raises(NotImplementedError, match="width 100 is off the grid"):
        pinit.mlp_hidden_width(*_kw([100, 100], [100, 100]).values())


@pytest.mark.parametrize("bad,what", [(0, "outside"), (-64, "outside"), (1025, "outside"), (2048, "outside"), (100.0, "no integer"),
                                      ("128", "no integer"), (True, "no integer"), (None, "no integer")])
def test_the_switch_refuses_what_lies_outside_1_to_1024(bad, what):
    for shapes, dims in ((True, [128, bad]), (False, [bad, bad])):
        with pytest.raises(NotImplementedError) as e:
            pinit.network_spec(*_kw(dims, [128, 128]).values(), None, A, mlp_shapes=shapes, mlp_ragged=True)
        assert what in str(e.value) and "served:" in str(e.value) and "any integer in [1, 1024] under mlp_ragged=True" in str(e.value), str(e.value)


def test_widths_on_the_grid_through_the_switch_are_the_call_without():
    for shapes, cd, pd in ((True, [128, 256, 64], [192]), (False, [320, 320], [320, 320]), (True, [192, 192], [192, 192])):
        a = pinit.network_spec(*_kw(cd, pd).values(), None, A, mlp_shapes=shapes, mlp_ragged=True)
        b = pinit.network_spec(*_kw(cd, pd).values(), None, A, mlp_shapes=shapes)
        assert a == b and not a.ragged and a.to_c().ragged_widths == 0


def test_dropout_beside_a_width_off_the_grid_is_refused():
    with pytest.raises(NotImplementedError, match="mlp_ragged=True with mlp_dropout=True and a positive dropout_rate"):
        pinit.network_spec(*_kw([100, 100], [100, 100], dropout_rate=0.1).values(), None, A, mlp_dropout=True, mlp_ragged=True)
    spec = pinit.network_spec(*_kw([128, 128], [128, 128], dropout_rate=0.1).values(), None, A, mlp_dropout=True, mlp_ragged=True)
    assert spec.critic_dropout == 0.1 and not spec.ragged        # on the grid: served as always
    spec = pinit.network_spec(*_kw([100, 100], [100, 100], dropout_rate=0.0).values(), None, A, mlp_dropout=True, mlp_ragged=True)
    assert spec.ragged


def test_to_c_default_leaves_the_field_zero():
    assert NetSpec().to_c().ragged_widths == 0 and NetSpec(ragged=True, hidden=100).to_c().ragged_widths == 1


def test_create_functions_take_the_switch(monkeypatch):
    from test_agent_opts_cpu import _spec_of
    kw = dict(mlp_shapes=True, mlp_ragged=True, **_kw([400, 300], [400, 300]))
    a, b = _spec_of("states", monkeypatch, **kw), _spec_of("drq", monkeypatch, **kw)
    assert a == b == NetSpec(hidden=400, critic_dims=(400, 300), policy_dims=(400, 300), ragged=True)
    kw.pop("mlp_ragged")
    a, b = _spec_of("states", monkeypatch, **kw), _spec_of("drq", monkeypatch, **kw)
    assert a == b and a[0] is NotImplementedError and "width 400" in a[1] and "off the grid" in a[1]


# ---- the C ABI: serl_agent_create_opts returns its argument errors before any device call ------------------------------------------
def _opts(cd, pd, ragged, **kw):
    return NetSpec(critic_dims=tuple(cd), policy_dims=tuple(pd), hidden=cd[0], ragged=bool(ragged), **kw).to_c()


def test_c_field_zero_is_todays_check_with_todays_message():
    o = _opts([400, 300], [64], 0)
    rc, msg = _create(o)
    assert rc == SERL_ERR_INVALID and "critic MLP: layer 1 has width 400 (served: 1 to 4 layers, each a multiple of 64 in [64, 1024] wide)" in msg, msg
    rc, msg = _create(NetSpec().to_c(), _cfg(hidden=100))
    assert rc == SERL_ERR_INVALID and "hidden must be a multiple of 64 in [64, 1024] (got 100)" in msg, msg


def test_c_field_one_admits_1_to_1024_and_refuses_the_rest():
    for cd, pd in (([400, 300], [400, 300]), ([1], [1024, 3, 50, 65]), ([64, 64], [64])):
        rc, msg = _create(_opts(cd, pd, 1))
        assert rc != SERL_ERR_INVALID, (cd, pd, msg)        # (made and destroyed where a device is present; a device error where none is)
    rc, msg = _create(NetSpec(ragged=True).to_c(), _cfg(hidden=100))
    assert rc != SERL_ERR_INVALID, msg
    for w in (0, -5, 1025):
        o = _opts([128, 64], [64], 1)
        o.critic.dims[1] = w
        rc, msg = _create(o)
        assert rc == SERL_ERR_INVALID and f"critic MLP: layer 2 has width {w}" in msg and "each in [1, 1024] wide" in msg, msg
        o = _opts([64], [128, 64], 1)
        o.policy.dims[0] = w
        rc, msg = _create(o)
        assert rc == SERL_ERR_INVALID and f"policy MLP: layer 1 has width {w}" in msg, msg
        rc, msg = _create(NetSpec(ragged=True).to_c(), _cfg(hidden=w))
        assert rc == SERL_ERR_INVALID and f"hidden must lie in [1, 1024] with ragged_widths 1 (got {w})" in msg, msg
    o = _opts([64], [64], 1)
    o.critic.n_layers = 5
    rc, msg = _create(o)
    assert rc == SERL_ERR_INVALID and "critic MLP: 5 hidden layers" in msg, msg


@pytest.mark.parametrize("value", [2, -1, 64])
def test_c_field_refuses_other_values_naming_field_and_value(value):
    o = _opts([64, 64], [64, 64], 0)
    o.ragged_widths = value
    rc, msg = _create(o)
    assert rc == SERL_ERR_INVALID and f"ragged_widths {value} is not" in msg, msg


def test_c_dropout_beside_a_width_off_the_grid_is_refused():
    o = NetSpec(hidden=100, ragged=True).to_c()
    o.critic.dropout = 0.1
    rc, msg = _create(o, _cfg(hidden=100))
    assert rc == SERL_ERR_INVALID and "beside an MLP width off the 64 grid" in msg and "dropout 0.1" in msg, msg
    o = NetSpec(hidden=128, ragged=True).to_c()        # on the grid: not this refusal
    o.critic.dropout = 0.1
    rc, msg = _create(o, _cfg(hidden=128))
    assert rc != SERL_ERR_INVALID, msg


def test_the_older_entry_points_leave_the_field_zero():
    from serl_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    dims = (C.c_int32 * 2)(400, 300)
    rc = int(L.serl_agent_create_shapes(C.byref(_cfg()), 0, 0, 0, 0, dims, 2, dims, 2, C.byref(h)))
    assert rc == SERL_ERR_INVALID and "critic MLP: layer 1 has width 400" in (L.serl_last_error() or b"").decode()


# ---- leaf tables and the flax tree at true shapes ------------------------------------------------------------------------------------
def test_leaf_tables_and_flax_tree_have_true_shapes():
    from serl_amd.agents.flax_tree import theta_paths, tree_from_leaves
    spec = pinit.network_spec(*_kw([400, 300], [50]).values(), None, A, mlp_shapes=True, mlp_ragged=True)
    sh = pinit.theta_shapes(0, 0, 0, 10, A, ensemble=2, **spec.leaf_kwargs())
    assert sh["critic/w1"] == (2, 14, 400) and sh["critic/w2"] == (2, 400, 300) and sh["critic/ln2/scale"] == (2, 300)
    assert sh["critic/head/kernel"] == (2, 300, 1) and sh["actor/w1"] == (10, 50) and sh["actor/mean/kernel"] == (50, A)
    theta = pinit.init_theta(0, 0, 0, 10, A, seed=3, ensemble=2, **spec.leaf_kwargs())
    assert {k: v.shape for k, v in theta.items()} == sh
    paths = theta_paths((), **{k: v for k, v in spec.leaf_kwargs().items()})
    tree = tree_from_leaves(paths, sh, lambda leaf: theta[leaf].reshape(-1))
    assert tree["modules_critic"]["network"]["Dense_1"]["kernel"].shape == (2, 400, 300)
    assert tree["modules_critic"]["network"]["LayerNorm_1"]["scale"].shape == (2, 300)
    assert tree["modules_actor"]["network"]["Dense_0"]["kernel"].shape == (10, 50)
    assert tree["modules_actor"]["Dense_0"]["kernel"].shape == (50, A)


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------
def test_oracle_of_the_case_table_at_h_h_is_the_shape_general_oracle():
    """the Config and the installed functions of tests/mlp_ragged.py at (128, 128) twice compute what tests/mlp_shapes.py's compute,
    bit for bit: one update_high_utd, every leaf of the state and the info"""
    import policy_fixed as PF
    B = 6
    out = []
    for cfg, inst, init in ((PF.FixedConfig(image_keys=(), S=10, A=4, discount=0.99, hidden=128, critic_dims=(128, 128), policy_dims=(128, 128)),
                             MR.installed, PF.init_params),
                            (MS.config("state", (128, 128), (128, 128)), MS.installed, MS.init_params)):
        with inst():
            st = O.TrainState(cfg, *init(cfg, 42), torch.float64)
            b, noise = AH.synth_batch(cfg, B, seed=4), O.make_noise(cfg, B, seed=8, utd_ratio=2)
            info, _ = O.update_high_utd(st, AH.batch_to_torch(b, torch.float64), O.noise_to_torch(noise, torch.float64), 2)
        out.append((st, info))
    (a, ia), (b, ib) = out
    assert ia == ib and list(a.params) == list(b.params)
    for k in a.params:
        assert torch.equal(a.params[k], b.params[k]) and torch.equal(a.target[k], b.target[k]), k


@pytest.mark.parametrize("name", [n for n in MR.IDS if "relu" in n])
def test_relu_cases_keep_their_distance_from_the_kink(name):
    with MR.installed():
        worst = MR.check_relu_margin(name)
    print(f"{name}: min |relu pre-activation| over its oracle runs = {worst:.3g}")


def test_case_table_covers_every_row_layout_with_a_ragged_tail():
    widths = {d for c in MR.CASES.values() for d in c["critic_dims"] + c["policy_dims"]}
    assert {50, 3} <= widths and 200 in widths and {65, 100, 127, 300, 400, 1000} <= widths
    assert {c["rows"] for c in MR.CASES.values()} <= {6, 65, 72}
    for name in MR.IDS:
        cfg, B, utd, _ = MR.case_config(name)
        assert (cfg.critic_dims, cfg.policy_dims) == (MR.CASES[name]["critic_dims"], MR.CASES[name]["policy_dims"])
        assert utd == 0 or B % utd == 0


# ---- the reference's own code (tests/golden/ragged_*.npz, tests/golden/make_golden_update_ragged.py) -------------------------------------
def _goldens():
    from oracle import golden_update as G
    out = [(f"update_{n}", MR.load_golden(n)) for n in MR.UPDATE_GOLDEN]
    z, cfg, _, _ = MR.init_golden()
    g = G.unpack(z)
    g["cfg"] = cfg
    return out + [("init_sac_state", g)]


@pytest.mark.parametrize("name,g", _goldens(), ids=[n for n, _ in _goldens()])
def test_paths_and_export_are_the_references_tree_at_true_widths(name, g):
    from oracle import golden_update as G
    from serl_amd.agents import flax_tree as FT
    from test_mlp_shapes_cpu import _ShapeCore
    cfg, want = g["cfg"], g["meta"]["param_tree"]
    assert g["meta"]["mlp_shapes"] == {"critic": list(cfg.critic_dims), "policy": list(cfg.policy_dims)}
    assert any(d % 64 for d in cfg.critic_dims + cfg.policy_dims)
    for mod, dims in (("modules_critic", cfg.critic_dims), ("modules_actor", cfg.policy_dims)):      # the reference's kernels: true widths
        assert [want[mod]["network"][f"Dense_{j}"]["kernel"][-1] for j in range(len(dims))] == list(dims)
    shapes = pinit.theta_shapes(cfg.n_cam, cfg.H, cfg.W, cfg.S, cfg.A, ensemble=cfg.ensemble, encoder_type=cfg.encoder_type,
                                critic_dims=cfg.critic_dims, policy_dims=cfg.policy_dims)
    assert [AH.product_name(k, cfg.image_keys) for k in MS.trainable_param_shapes(cfg)] == list(shapes)     # arena order
    assert G.shape_tree(FT.export_tree(_ShapeCore(cfg), "params", cfg.image_keys)) == want


def test_host_twins_equal_the_reference_initial_params_at_true_widths():
    import init_golden_helpers as IG
    from serl_amd.utils import init_ref as IR
    z, cfg, recs, shapes = MR.init_golden()
    assert cfg.critic_dims == (100, 50) and cfg.policy_dims == (65, 127, 3)
    assert shapes["actor/w3"] == (127, 3) and shapes["critic/w2"] == (cfg.ensemble, 100, 50) and shapes["critic/head/kernel"] == (cfg.ensemble, 50, 1)
    got = IR.theta_reference(cfg.image_keys, cfg.H, cfg.W, cfg.S, cfg.A, 0, ensemble=cfg.ensemble, encoder_type=cfg.encoder_type,
                             temperature_init=1e-2, device=None, critic_dims=cfg.critic_dims, policy_dims=cfg.policy_dims)
    assert set(got) == set(recs), sorted(set(got) ^ set(recs))
    bad = [m for m in (IG.mismatch(n, recs[n], got[n]) for n in sorted(recs)) if m]
    assert not bad, bad
    for n, v in got.items():
        assert tuple(v.shape) == shapes[n], (n, v.shape, shapes[n])


@pytest.mark.parametrize("name", MR.UPDATE_GOLDEN)
def test_general_oracle_reproduces_the_reference_golden(name):
    from oracle import golden_update as G
    from test_mlp_shapes_cpu import F64_TOL, _oracle_sections, _run_oracle
    g = MR.load_golden(name)
    cfg = g["cfg"]
    with MS.installed():
        st, infos = _run_oracle(cfg, g["steps"], g["meta"]["param_seed"])
        for i, (info, step) in enumerate(zip(infos, g["steps"])):
            for k, v in info.items():
                r = step["info"][k]
                assert abs(v - r) <= F64_TOL * max(1.0, abs(r)), (i, k, v, r)
        assert st.step == g["meta"]["final_step"]
        worst = 0.0
        for sec, tree in _oracle_sections(st).items():
            assert set(g["final"][sec]) == set(tree), sec
            for leaf, t in tree.items():
                e, how = G.leaf_compare(f"{sec}/{leaf}", g["final"][sec][leaf], t.numpy())
                assert e < F64_TOL, (sec, leaf, how, e)
                worst = max(worst, e)
    print(f"ragged_update_{name}: general oracle vs reference golden, worst {worst:.1e}")
