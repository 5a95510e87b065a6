"""CPU: critic and policy MLPs of their own depth and per-layer widths (mlp_shapes=True; hidden_dims of 1 to 4 layers per network).

* the shape-general oracle functions of tests/mlp_shapes.py equal the originals bit for bit at [h, h], and reproduce the reference's
  own update code on tests/golden/shapes_update_*.npz within the F64_TOL of tests/test_reference_update.py;
* utils.init.mlp_layer_dims reads what it is given and refuses, from the arguments alone, what is not served; without the switch
  every refusal of tests/test_mlp_widths_cpu.py still stands;
* theta_shapes / theta_paths / export_tree give the tree the reference really built (the goldens' param_tree);
* init_ref's host twins equal the reference's initial parameters of shapes_init_sac_state.npz bit for bit."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import drq_oracle as O
from oracle import golden_update as G
import agent_helpers as AH
import init_golden_helpers as IG
import mlp_shapes as MS
from serl_amd.agents import flax_tree as FT
from serl_amd.utils import init as pinit
from serl_amd.utils import init_ref as IR
from test_mlp_widths_cpu import REFUSALS, _create_drq, _create_states
from test_reference_update import F64_TOL, _oracle_sections, _run_oracle


# ---- the general oracle at [h, h] is the oracle ----------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [64, 256, 320])
@pytest.mark.parametrize("kind", ["state", "small"])
def test_general_oracle_equals_the_original_at_h_h(h, kind):
    kw = dict(image_keys=(), S=10, A=4, discount=0.99) if kind == "state" else dict(image_keys=("wrist",), H=33, W=47, S=5, A=3, encoder_type="small")
    cfg = O.Config(hidden=h, ensemble=3, **kw)
    B = 6
    assert list(MS.trainable_param_shapes(cfg).items()) == list(O.trainable_param_shapes(cfg).items())
    want, got = O.init_params(cfg, 11), MS.init_params(cfg, 11)
    for w, g_ in zip(want, got):
        assert list(w) == list(g_)
        for k in w:
            assert np.array_equal(np.asarray(w[k]).view(np.uint32), np.asarray(g_[k]).view(np.uint32)), k
    b = AH.batch_to_torch(AH.synth_batch(cfg, B, seed=3), torch.float64)
    noise = O.noise_to_torch(O.make_noise(cfg, B, seed=7, utd_ratio=2), torch.float64)
    st0 = O.TrainState(cfg, *want, torch.float64)
    info0, aux0 = O.update_high_utd(st0, b, noise, 2)
    with MS.installed():
        assert O.critic_forward is MS.critic_forward
        st1 = O.TrainState(cfg, *got, torch.float64)
        info1, aux1 = O.update_high_utd(st1, b, noise, 2)
    assert O.critic_forward is not MS.critic_forward and O.init_params is not MS.init_params
    assert info0 == info1
    for k, v in aux0["g_actor"].items():
        assert torch.equal(v, aux1["g_actor"][k]), k
    for sec, tree in _oracle_sections(st0).items():
        for leaf, t in tree.items():
            assert torch.equal(t, _oracle_sections(st1)[sec][leaf]), (sec, leaf)


# ---- the Python interface ---------------------------------------------------------------------------------------------------------
def test_mlp_layer_dims_reads_the_two_lists():
    assert pinit.mlp_layer_dims(None, None) == ((256, 256), (256, 256))
    assert pinit.mlp_layer_dims({}, {"activations": "tanh"}) == ((256, 256), (256, 256))
    assert pinit.mlp_layer_dims(MS.mlp_kwargs([512, 512, 512]), MS.mlp_kwargs([256, 256])) == ((512, 512, 512), (256, 256))
    assert pinit.mlp_layer_dims(MS.mlp_kwargs((64,)), MS.mlp_kwargs(np.array([1024, 64, 128, 192]))) == ((64,), (1024, 64, 128, 192))
    assert pinit.MAX_MLP_LAYERS == 4
    assert pinit.resolve_mlp_dims(192) == ((192, 192), (192, 192)) and pinit.resolve_mlp_dims(192, [64], None) == ((64,), (192, 192))


SHAPE_REFUSALS = [
    ("no_layer_norm", dict(critic_network_kwargs=MS.mlp_kwargs([128], use_layer_norm=False)), "critic_network_kwargs: use_layer_norm=False"),
    ("no_layers", dict(policy_network_kwargs=MS.mlp_kwargs([])), r"policy_network_kwargs: hidden_dims=\[\] has 0 layers"),
    ("five_layers", dict(critic_network_kwargs=MS.mlp_kwargs([64] * 5)), "critic_network_kwargs: hidden_dims=.* has 5 layers"),
    ("off_the_grid_100", dict(policy_network_kwargs=MS.mlp_kwargs([128, 100])), "policy_network_kwargs: width 100 in hidden_dims=.* is off the grid"),
    ("off_the_grid_1088", dict(critic_network_kwargs=MS.mlp_kwargs([1088])), "critic_network_kwargs: width 1088 in hidden_dims=.* is off the grid"),
    ("off_the_grid_0", dict(critic_network_kwargs=MS.mlp_kwargs([0, 64])), "critic_network_kwargs: width 0 in hidden_dims=.* is off the grid"),
    ("not_an_integer", dict(policy_network_kwargs=MS.mlp_kwargs([128.0, 64])), "policy_network_kwargs: width 128.0 in hidden_dims=.* is no integer"),
    ("a_string", dict(policy_network_kwargs=MS.mlp_kwargs(["128"])), "policy_network_kwargs: width '128' in hidden_dims=.* is no integer"),
]


@pytest.mark.parametrize("create", [_create_states, _create_drq], ids=["create_states", "create_drq"])
@pytest.mark.parametrize("kw,message", [r[1:] for r in SHAPE_REFUSALS], ids=[r[0] for r in SHAPE_REFUSALS])
def test_shape_refusals_say_what_is_served(create, kw, message):
    """raised from the arguments alone: no device is touched (this test runs without one)"""
    with pytest.raises(NotImplementedError, match=message) as e:
        create(policy_kwargs=dict(MS.POLICY_KWARGS), mlp_shapes=True, **kw)
    assert "served: hidden_dims of 1 to 4 layers with LayerNorm, every width a multiple of 64 in [64, 1024], the critic's list " \
           "independent of the policy's" in str(e.value)


@pytest.mark.parametrize("create", [_create_states, _create_drq], ids=["create_states", "create_drq"])
@pytest.mark.parametrize("kw,message", [r[1:] for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_without_the_switch_every_old_refusal_stands(create, kw, message):
    for extra in ({}, {"mlp_shapes": False}):
        with pytest.raises(NotImplementedError, match=message) as e:
            create(policy_kwargs=dict(MS.POLICY_KWARGS), **kw, **extra)
        assert "served: hidden_dims=[h, h] with LayerNorm, h a multiple of 64 in [64, 1024], the same h for critic and policy" in str(e.value)


@pytest.mark.parametrize("create", [_create_states, _create_drq], ids=["create_states", "create_drq"])
def test_dropout_with_other_shapes_is_refused(create):
    for cd, pd in (([128, 256], [128, 256]), ([128, 128], [64, 64]), ([128, 128, 128], [128, 128, 128]), ([128], [128])):
        with pytest.raises(NotImplementedError, match="mlp_shapes=True with mlp_dropout=True") as e:
            create(policy_kwargs=dict(MS.POLICY_KWARGS), mlp_shapes=True, mlp_dropout=True,
                   critic_network_kwargs=MS.mlp_kwargs(cd, dropout_rate=0.1), policy_network_kwargs=MS.mlp_kwargs(pd))
        assert "hidden_dims=[h, h], the same in both networks" in str(e.value)
    pinit.NetSpec(critic_dims=(128, 128), policy_dims=(128, 128), critic_dropout=0.1).check()      # one [h, h]: served
    pinit.NetSpec(critic_dims=(128, 256, 64), policy_dims=(64,)).check()                           # no positive rate: served


# ---- shapes, paths and the exported tree against the tree the reference built ----------------------------------------------------
class _ShapeCore:
    """what export_tree reads of a core: cfg, the two lists, and get(section, leaf) -> the leaf's flat values"""

    def __init__(self, cfg):
        self.cfg = SimpleNamespace(n_cam=cfg.n_cam, H=cfg.H, W=cfg.W, state_dim=cfg.S, act_dim=cfg.A, ensemble=cfg.ensemble,
                                   hidden=cfg.hidden, encoder_type=1 if cfg.encoder_type == "small" else 0, num_stack=1)
        self.critic_dims, self.policy_dims = cfg.critic_dims, cfg.policy_dims
        self.shapes = dict(pinit.theta_shapes(cfg.n_cam, cfg.H, cfg.W, cfg.S, cfg.A, ensemble=cfg.ensemble, encoder_type=cfg.encoder_type,
                                              critic_dims=cfg.critic_dims, policy_dims=cfg.policy_dims), **FT.trunk_shapes())

    def get(self, section, leaf):
        return np.zeros(int(np.prod(self.shapes[leaf])), np.float32)


def _goldens():
    out = [(f"update_{n}", MS.load_golden(n)) for n in MS.UPDATE_GOLDEN]
    z, cfg, _, _ = MS.init_golden()
    g = G.unpack(z)
    g["cfg"] = cfg
    return out + [("init_sac_state", g)]


@pytest.mark.parametrize("name,g", _goldens(), ids=[n for n, _ in _goldens()])
def test_shapes_paths_and_export_are_the_references_tree(name, g):
    cfg, want = g["cfg"], g["meta"]["param_tree"]
    assert g["meta"]["mlp_shapes"] == {"critic": list(cfg.critic_dims), "policy": list(cfg.policy_dims)}
    shapes = pinit.theta_shapes(cfg.n_cam, cfg.H, cfg.W, cfg.S, cfg.A, ensemble=cfg.ensemble, encoder_type=cfg.encoder_type,
                                critic_dims=cfg.critic_dims, policy_dims=cfg.policy_dims)
    paths = FT.theta_paths(cfg.image_keys, encoder_type=cfg.encoder_type, critic_dims=cfg.critic_dims, policy_dims=cfg.policy_dims)
    assert list(paths) and set(paths) == set(shapes)
    assert [AH.product_name(k, cfg.image_keys) for k in MS.trainable_param_shapes(cfg)] == list(shapes)     # arena order
    for leaf, ps in paths.items():
        node = want
        for p in ps[0]:
            node = node[p]
        assert list(node) == list(shapes[leaf]) or int(np.prod(node)) == int(np.prod(shapes[leaf])), (leaf, node, shapes[leaf])
    for net, dims in (("modules_critic", cfg.critic_dims), ("modules_actor", cfg.policy_dims)):
        mods = want[net]["network"]
        assert sorted(mods) == sorted([f"Dense_{j}" for j in range(len(dims))] + [f"LayerNorm_{j}" for j in range(len(dims))])
    tree = FT.export_tree(_ShapeCore(cfg), "params", cfg.image_keys)
    assert G.shape_tree(tree) == want


def test_two_layer_tables_are_unchanged():
    for n_cam, H, W in ((0, 0, 0), (2, 64, 64)):
        old = pinit.theta_shapes(n_cam, H, W, 7, 3, hidden=192)
        new = pinit.theta_shapes(n_cam, H, W, 7, 3, hidden=64, critic_dims=(192, 192), policy_dims=(192, 192))
        assert list(old.items()) == list(new.items())
        a, b = pinit.init_theta(n_cam, H, W, 7, 3, seed=5, hidden=192), pinit.init_theta(n_cam, H, W, 7, 3, seed=5, critic_dims=(192, 192), policy_dims=(192, 192))
        assert list(a) == list(b) and all(np.array_equal(a[k], b[k]) for k in a)
    keys = ("front", "wrist")
    assert FT.theta_paths(keys) == FT.theta_paths(keys, critic_dims=(64, 128), policy_dims=(128, 64))
    assert FT.theta_paths(()) == FT.theta_paths((), critic_dims=(64, 128), policy_dims=(128, 64))


# ---- the reference's initial parameters and update code ------------------------------------------------------------------------------
def test_host_twins_equal_the_reference_initial_params():
    z, cfg, recs, shapes = MS.init_golden()
    assert cfg.critic_dims == (128, 64) and cfg.policy_dims == (64, 64, 128)
    assert shapes["actor/w3"] == (64, 128) and shapes["critic/w2"] == (cfg.ensemble, 128, 64) and shapes["critic/head/kernel"] == (cfg.ensemble, 64, 1)
    got = IR.theta_reference(cfg.image_keys, cfg.H, cfg.W, cfg.S, cfg.A, 0, ensemble=cfg.ensemble, encoder_type=cfg.encoder_type,
                             temperature_init=1e-2, device=None, critic_dims=cfg.critic_dims, policy_dims=cfg.policy_dims)
    assert set(got) == set(recs), sorted(set(got) ^ set(recs))
    bad = [m for m in (IG.mismatch(n, recs[n], got[n]) for n in sorted(recs)) if m]
    assert not bad, bad
    for n, v in got.items():
        assert tuple(v.shape) == shapes[n], (n, v.shape, shapes[n])
    assert np.array_equal(IR.create_rng_of(0), z["init_rng"])      # state.rng after create does not depend on the shapes


@pytest.mark.parametrize("name", MS.UPDATE_GOLDEN)
def test_general_oracle_reproduces_the_reference_golden(name):
    g = MS.load_golden(name)
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
    print(f"shapes_update_{name}: general oracle vs reference golden, worst {worst:.1e}")
