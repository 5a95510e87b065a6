"""CPU: critic and policy MLPs of a width other than 256 (hidden_dims=[h, h], h a multiple of 64 in [64, 1024]).

* tests/golden/widths_update_*.npz were produced by tests/golden/make_golden_update_widths.py from the reference's own update
  code with its create functions' hidden_dims overridden; the fp64 oracle at Config(hidden=h) reproduces them within the bound of
  tests/test_reference_update.py, which pins the fixtures the GPU tests compare with.
* utils/init_ref.py's host twins at width 128 equal the parameters the reference's create_states draws from seed 0
  (widths_init_sac_state_w128.npz, bit for bit), as tests/test_init_reference_cpu.py checks at 256.
* theta_shapes / theta_paths / export_tree give the reference's parameter tree at any width.
* create_drq / create_states refuse what is not served before they touch a device."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import drq_oracle as O
from oracle import golden_update as G
import golden_replay as GR
import init_golden_helpers as IG
import mlp_widths as MW
from serl_amd.agents import flax_tree as FT
from serl_amd.utils import init as pinit
from serl_amd.utils import init_ref as IR
from test_reference_update import F64_TOL, _oracle_sections, _run_oracle


@pytest.mark.parametrize("name", MW.UPDATE_GOLDEN)
def test_oracle_reproduces_the_reference_golden_at_other_widths(name):
    g = GR.load_variant("widths_update", name)[0]
    cfg = g["cfg"]
    assert cfg.hidden == int(name.rsplit("_w", 1)[1])
    assert g["meta"]["param_tree"]["modules_actor"]["network"]["Dense_1"]["kernel"] == [cfg.hidden, cfg.hidden]
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
    print(f"widths_update_{name}: oracle vs reference golden, worst {worst:.1e}")


def test_host_twins_equal_the_reference_initial_params_at_width_128():
    z, cfg, recs, shapes = MW.init_golden()
    assert cfg.hidden == 128 and shapes["actor/w2"] == (128, 128) and shapes["critic/w1"] == (cfg.ensemble, cfg.S + cfg.A, 128)
    got = IR.theta_reference(cfg.image_keys, cfg.H, cfg.W, cfg.S, cfg.A, 0, ensemble=cfg.ensemble, encoder_type=cfg.encoder_type,
                             temperature_init=1e-2, device=None, hidden=cfg.hidden)
    assert set(got) == set(recs), sorted(set(got) ^ set(recs))
    bad = [m for m in (IG.mismatch(n, recs[n], got[n]) for n in sorted(recs)) if m]
    assert not bad, bad
    for n, v in got.items():
        assert tuple(v.shape) == shapes[n], (n, v.shape, shapes[n])
    assert np.array_equal(IR.create_rng_of(0), z["init_rng"])      # state.rng after create does not depend on the width
    # the leaves carry the width's own fans: the default width draws other values under the same keys
    base = IR.theta_reference((), 0, 0, cfg.S, cfg.A, 0, ensemble=cfg.ensemble, temperature_init=1e-2, device=None)
    assert base["actor/w2"].shape == (256, 256)
    assert {lf.name: lf.shape for lf in IR.theta_leaves((), 0, 0, cfg.S, cfg.A, ensemble=cfg.ensemble, hidden=128)} == \
        {k: tuple(v) for k, v in pinit.theta_shapes(0, 0, 0, cfg.S, cfg.A, ensemble=cfg.ensemble, hidden=128).items()}


def _at_width(tree, h_from, h_to, path=()):
    """The golden's recorded shape tree at another hidden width.  Where the width sits follows from the flax modules alone
    (networks/mlp.py, actor_critic_nets.py): in the MLP ("network") Dense_0's kernel is (in, h), Dense_1's (h, h), every bias and
    LayerNorm vector (h,); the Dense heads behind an MLP have kernels (h, out).  Nothing under "encoder" depends on it (the
    one-camera encoding is 320 wide, like the golden's MLP: a substitution by value would be wrong)."""
    if isinstance(tree, dict):
        return {k: _at_width(v, h_from, h_to, path + (k,)) for k, v in tree.items()}
    shp = list(tree)
    if "encoder" in path:
        return shp
    leaf, mod = path[-1], path[-2]
    if "network" in path:
        at = (-2, -1) if (leaf == "kernel" and mod == "Dense_1") else (-1,)
    elif leaf == "kernel" and mod.startswith("Dense_"):
        at = (-2,)
    else:
        at = ()
    for i in at:
        assert shp[i] == h_from, (path, shp)
        shp[i] = h_to
    return shp


class _ShapeCore:
    """what export_tree reads of a core: cfg and get(section, leaf) -> the leaf's flat values"""

    def __init__(self, cfg, hidden):
        self.cfg = SimpleNamespace(n_cam=cfg.n_cam, H=cfg.H, W=cfg.W, state_dim=cfg.S, act_dim=cfg.A, ensemble=cfg.ensemble,
                                   hidden=hidden, encoder_type=1 if cfg.encoder_type == "small" else 0, num_stack=1)
        self.shapes = dict(pinit.theta_shapes(cfg.n_cam, cfg.H, cfg.W, cfg.S, cfg.A, ensemble=cfg.ensemble, hidden=hidden,
                                              encoder_type=cfg.encoder_type), **FT.trunk_shapes())

    def get(self, section, leaf):
        return np.zeros(int(np.prod(self.shapes[leaf])), np.float32)


@pytest.mark.parametrize("name", MW.UPDATE_GOLDEN)
@pytest.mark.parametrize("h", [64, 320, 1024])
def test_shapes_paths_and_export_follow_the_width(name, h):
    g = GR.load_variant("widths_update", name)[0]
    cfg = g["cfg"]
    want = _at_width(g["meta"]["param_tree"], cfg.hidden, h)
    shapes = pinit.theta_shapes(cfg.n_cam, cfg.H, cfg.W, cfg.S, cfg.A, ensemble=cfg.ensemble, hidden=h, encoder_type=cfg.encoder_type)
    paths = FT.theta_paths(cfg.image_keys, encoder_type=cfg.encoder_type)
    assert set(paths) == set(shapes)
    for leaf, ps in paths.items():
        node = want
        for p in ps[0]:
            node = node[p]
        assert int(np.prod(node)) == int(np.prod(shapes[leaf])), (leaf, node, shapes[leaf])
    tree = FT.export_tree(_ShapeCore(cfg, h), "params", cfg.image_keys)
    assert G.shape_tree(tree) == want


def _create_states(**kw):
    from serl_amd.agents.sac import SACAgent
    return SACAgent.create_states(0, np.zeros((10,), np.float32), np.zeros((4,), np.float32), **kw)


def _create_drq(**kw):
    from serl_amd.agents.drq import DrQAgent
    obs = {"image": np.zeros((1, 64, 64, 3), np.uint8), "state": np.zeros((1, 5), np.float32)}
    return DrQAgent.create_drq(0, obs, np.zeros((3,), np.float32), encoder_type="resnet-pretrained", use_proprio=True,
                               image_keys=("image",), **kw)


REFUSALS = [
    ("two_layer_widths", dict(critic_network_kwargs=MW.mlp_kwargs(128, hidden_dims=[128, 256]), policy_network_kwargs=MW.mlp_kwargs(128)),
     "two different layer widths"),
    ("critic_and_policy_differ", dict(critic_network_kwargs=MW.mlp_kwargs(512), policy_network_kwargs=MW.mlp_kwargs(128)),
     "critic width 512 and policy width 128 differ"),
    ("policy_alone_differs_from_the_default", dict(policy_network_kwargs=MW.mlp_kwargs(128)), "critic width 256 and policy width 128 differ"),
    ("three_layers", dict(critic_network_kwargs=MW.mlp_kwargs(128, hidden_dims=[128, 128, 128]), policy_network_kwargs=MW.mlp_kwargs(128)),
     "has 3 layers"),
    ("one_layer", dict(critic_network_kwargs=MW.mlp_kwargs(128), policy_network_kwargs=MW.mlp_kwargs(128, hidden_dims=[128])),
     "has 1 layers"),
    ("no_layer_norm", dict(critic_network_kwargs=MW.mlp_kwargs(128, use_layer_norm=False), policy_network_kwargs=MW.mlp_kwargs(128)),
     "use_layer_norm=False"),
    ("off_the_grid_100", dict(critic_network_kwargs=MW.mlp_kwargs(100), policy_network_kwargs=MW.mlp_kwargs(100)), "width 100 is off the grid"),
    ("off_the_grid_1088", dict(critic_network_kwargs=MW.mlp_kwargs(1088), policy_network_kwargs=MW.mlp_kwargs(1088)), "width 1088 is off the grid"),
    ("off_the_grid_0", dict(critic_network_kwargs=MW.mlp_kwargs(0), policy_network_kwargs=MW.mlp_kwargs(0)), "width 0 is off the grid"),
]


@pytest.mark.parametrize("create", [_create_states, _create_drq], ids=["create_states", "create_drq"])
@pytest.mark.parametrize("kw,message", [r[1:] for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_refusals_say_what_is_served(create, kw, message):
    """raised from the arguments alone: no device is touched (this test runs without one)"""
    with pytest.raises(NotImplementedError, match=message) as e:
        create(policy_kwargs=dict(MW.POLICY_KWARGS), **kw)
    assert "served: hidden_dims=[h, h] with LayerNorm, h a multiple of 64 in [64, 1024], the same h for critic and policy" in str(e.value)


def test_width_grid():
    assert pinit.HIDDEN_WIDTHS == tuple(range(64, 1025, 64)) and len(pinit.HIDDEN_WIDTHS) == 16
    for h in pinit.HIDDEN_WIDTHS:
        assert pinit.mlp_hidden_width(MW.mlp_kwargs(h), MW.mlp_kwargs(h)) == h
    assert pinit.mlp_hidden_width(None, None) == 256 and pinit.mlp_hidden_width({}, {"activations": "tanh"}) == 256
