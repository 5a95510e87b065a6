"""CPU: critic and policy MLPs without LayerNorm (mlp_plain=True; use_layer_norm=False per network, mlp.py:29-30).

* utils.init.mlp_layer_norms reads what it is given and refuses what is no bool; Dropout beside a plain network is refused naming
  both switches; without the switch the old refusal still stands;
* theta_shapes, flax_tree.theta_paths, init_theta and init_ref's host twins hold no LayerNorm leaf for a plain network and all of
  them for the other; with both flags True they return what they return today;
* the general oracle functions of tests/mlp_plain.py equal the mlp_shapes ones bit for bit at both flags True, and reproduce the
  reference's own update code on tests/golden/plain_update_*.npz within the F64_TOL of tests/test_reference_update.py;
* every relu pre-activation of the GPU case table stays RELU_MARGIN from 0 on the fp64 oracle."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import drq_oracle as O
from oracle import golden_update as G
import agent_helpers as AH
import init_golden_helpers as IG
import mlp_plain as MP
import mlp_shapes as MS
from serl_amd.agents import flax_tree as FT
from serl_amd.utils import init as pinit
from serl_amd.utils import init_ref as IR
from test_mlp_widths_cpu import _create_drq, _create_states
from test_reference_update import F64_TOL, _oracle_sections, _run_oracle

CREATE = pytest.mark.parametrize("create", [_create_states, _create_drq], ids=["create_states", "create_drq"])


# ---- the argument reader ---------------------------------------------------------------------------------------------------------
def test_mlp_layer_norms_reads_one_flag_per_network():
    assert pinit.mlp_layer_norms(None, None) == (True, True)
    assert pinit.mlp_layer_norms({}, {"activations": "tanh"}) == (True, True)      # absent: what the launcher writes
    assert pinit.mlp_layer_norms({"use_layer_norm": False}, {"use_layer_norm": True}) == (False, True)
    assert pinit.mlp_layer_norms({"use_layer_norm": True}, {"use_layer_norm": np.bool_(False)}) == (True, False)
    assert pinit.mlp_layer_norms(MP.mlp_kwargs([64], False), MP.mlp_kwargs([64, 64], False)) == (False, False)
    for bad in (0, 1, None, "False", 0.0, [False]):
        for which in ("critic", "policy"):
            kw = {f"{which}_network_kwargs": {"use_layer_norm": bad}}
            with pytest.raises(NotImplementedError, match=f"{which}_network_kwargs: use_layer_norm=.*served: True or False"):
                pinit.mlp_layer_norms(kw.get("critic_network_kwargs"), kw.get("policy_network_kwargs"))


@CREATE
def test_a_flag_that_is_no_bool_is_refused_from_the_arguments_alone(create):
    with pytest.raises(NotImplementedError, match="policy_network_kwargs: use_layer_norm=0 "):
        create(policy_kwargs=dict(MS.POLICY_KWARGS), mlp_plain=True, policy_network_kwargs={"use_layer_norm": 0})


@CREATE
def test_dropout_beside_a_plain_network_is_refused_naming_both_switches(create):
    """raised from the arguments alone: no device is touched (this test runs without one)"""
    for ck, pk, where in ((MP.mlp_kwargs([128, 128], False, dropout_rate=0.1), MP.mlp_kwargs([128, 128], True), "critic_network_kwargs: use_layer_norm=False"),
                          (MP.mlp_kwargs([128, 128], True), MP.mlp_kwargs([128, 128], False, dropout_rate=0.2), "policy_network_kwargs: use_layer_norm=False"),
                          (MP.mlp_kwargs([128, 128], True, dropout_rate=0.1), MP.mlp_kwargs([128, 128], False), "critic_network_kwargs: dropout_rate=0.1")):
        with pytest.raises(NotImplementedError, match=where) as e:
            create(policy_kwargs=dict(MS.POLICY_KWARGS), mlp_plain=True, mlp_dropout=True, critic_network_kwargs=ck, policy_network_kwargs=pk)
        assert "mlp_plain=True" in str(e.value) and "mlp_dropout=True" in str(e.value)
    pinit.NetSpec(critic_dropout=0.1, policy_dropout=0.2).check()                      # LayerNorm in both: Dropout's own business
    pinit.NetSpec(critic_layer_norm=False, policy_layer_norm=False).check()            # no positive rate: served


@CREATE
def test_without_the_switch_the_old_refusal_stands(create):
    for shapes, served in ((False, "served: hidden_dims=[h, h] with LayerNorm, h a multiple of 64 in [64, 1024], the same h for critic and policy"),
                           (True, "served: hidden_dims of 1 to 4 layers with LayerNorm, every width a multiple of 64 in [64, 1024], the "
                                  "critic's list independent of the policy's")):
        for extra in ({}, {"mlp_plain": False}):
            with pytest.raises(NotImplementedError, match="critic_network_kwargs: use_layer_norm=False") as e:
                create(policy_kwargs=dict(MS.POLICY_KWARGS), mlp_shapes=shapes, critic_network_kwargs=MP.mlp_kwargs([128, 128], False),
                       policy_network_kwargs=MP.mlp_kwargs([128, 128], True), **extra)
            assert served in str(e.value) and "mlp_plain=True" in str(e.value)


def test_the_switch_leaves_the_other_refusals_alone():
    with pytest.raises(NotImplementedError, match="has 3 layers"):
        pinit.mlp_hidden_width(MP.mlp_kwargs([128, 128, 128], False), MP.mlp_kwargs([128, 128], False), mlp_plain=True)
    with pytest.raises(NotImplementedError, match="width 100 in hidden_dims=.* is off the grid"):
        pinit.mlp_layer_dims(MP.mlp_kwargs([100], False), None, mlp_plain=True)
    assert pinit.mlp_hidden_width(MP.mlp_kwargs([128, 128], False), MP.mlp_kwargs([128, 128], True), mlp_plain=True) == 128
    assert pinit.mlp_layer_dims(MP.mlp_kwargs([64], False), MP.mlp_kwargs([64, 128], False), mlp_plain=True) == ((64,), (64, 128))


# ---- shapes and trees ------------------------------------------------------------------------------------------------------------
def _is_ln(net, leaf):
    return leaf.startswith(f"{net}/ln")


@pytest.mark.parametrize("n_cam,H,W,etype", [(0, 0, 0, "resnet-pretrained"), (2, 64, 64, "resnet-pretrained"), (1, 64, 64, "small")])
@pytest.mark.parametrize("cln,pln", [(False, False), (False, True), (True, False)])
def test_no_layer_norm_leaf_for_a_plain_network_and_all_for_the_other(n_cam, H, W, etype, cln, pln):
    keys = ("front", "wrist")[:n_cam]
    cd, pd = (128, 64, 320), (64,)
    kw = dict(critic_dims=cd, policy_dims=pd)
    full = pinit.theta_shapes(n_cam, H, W, 7, 3, ensemble=3, encoder_type=etype, **kw)
    got = pinit.theta_shapes(n_cam, H, W, 7, 3, ensemble=3, encoder_type=etype, critic_layer_norm=cln, policy_layer_norm=pln, **kw)
    gone = [k for k in full if (not cln and _is_ln("critic", k)) or (not pln and _is_ln("actor", k))]
    assert len(gone) == 2 * ((0 if cln else len(cd)) + (0 if pln else len(pd)))
    assert list(got.items()) == [(k, v) for k, v in full.items() if k not in gone]          # the others, in the arena's order
    assert all(k in got for k in full if k.startswith("enc/") and "/ln/" in k) and (n_cam == 0 or "enc/proprio/ln/scale" in got)
    paths = FT.theta_paths(keys, encoder_type=etype, critic_layer_norm=cln, policy_layer_norm=pln, **kw)
    full_paths = FT.theta_paths(keys, encoder_type=etype, **kw)
    assert set(paths) == set(got) and all(paths[k] == full_paths[k] for k in paths)
    for net, mod, ln in (("critic", "modules_critic", cln), ("actor", "modules_actor", pln)):
        names = {p[0][2] for k, p in paths.items() if k.startswith(f"{net}/") and p[0][:2] == (mod, "network")}
        assert any(n.startswith("LayerNorm_") for n in names) == ln, (net, names)
    # both initialisers: the same Dense leaves as the LayerNorm agent of the seed, the LayerNorm leaves of the plain network absent
    a = pinit.init_theta(n_cam, H, W, 7, 3, seed=5, ensemble=3, encoder_type=etype, **kw)
    b = pinit.init_theta(n_cam, H, W, 7, 3, seed=5, ensemble=3, encoder_type=etype, critic_layer_norm=cln, policy_layer_norm=pln, **kw)
    assert list(b) == list(got) and all(np.array_equal(a[k], b[k]) for k in b)
    if n_cam == 0:
        ra = IR.theta_reference(keys, H, W, 7, 3, 0, ensemble=3, encoder_type=etype, device=None, **kw)
        rb = IR.theta_reference(keys, H, W, 7, 3, 0, ensemble=3, encoder_type=etype, device=None, critic_layer_norm=cln, policy_layer_norm=pln, **kw)
        assert list(rb) == list(got) and all(np.array_equal(ra[k], rb[k]) for k in rb)


def test_both_flags_true_return_what_they_return_today():
    for n_cam, H, W in ((0, 0, 0), (2, 64, 64)):
        keys = ("front", "wrist")[:n_cam]
        for kw in ({"hidden": 192}, {"critic_dims": (128, 64), "policy_dims": (64,)}):
            old, new = pinit.theta_shapes(n_cam, H, W, 7, 3, **kw), pinit.theta_shapes(n_cam, H, W, 7, 3, critic_layer_norm=True, policy_layer_norm=True, **kw)
            assert list(old.items()) == list(new.items())
            a = pinit.init_theta(n_cam, H, W, 7, 3, seed=5, **kw)
            b = pinit.init_theta(n_cam, H, W, 7, 3, seed=5, critic_layer_norm=True, policy_layer_norm=True, **kw)
            assert list(a) == list(b) and all(np.array_equal(a[k], b[k]) for k in a)
        assert FT.theta_paths(keys) == FT.theta_paths(keys, critic_layer_norm=True, policy_layer_norm=True)
    assert [lf for lf in IR.theta_leaves((), 0, 0, 7, 3, hidden=128)] == \
        [lf for lf in IR.theta_leaves((), 0, 0, 7, 3, hidden=128, critic_layer_norm=True, policy_layer_norm=True)]
    bare = FT.net_spec_of(SimpleNamespace(cfg=SimpleNamespace()))        # a core made before the flags existed
    assert (bare.critic_layer_norm, bare.policy_layer_norm) == (True, True)


# ---- the general oracle at both flags True is the mlp_shapes oracle ------------------------------------------------------------
@pytest.mark.parametrize("kind,cd,pd", [("state", (128, 64), (64,)), ("small", (64, 64), (64, 64))])
def test_general_oracle_equals_the_shapes_oracle_with_layer_norm_in_both(kind, cd, pd):
    cfg_s = MS.config(kind, cd, pd, ensemble=3, critic_activation="swish")
    cfg_p = MP.config(kind, cd, pd, True, True, ensemble=3, critic_activation="swish")
    B = 6
    assert list(MP.trainable_param_shapes(cfg_p).items()) == list(MS.trainable_param_shapes(cfg_s).items())
    want, got = MS.init_params(cfg_s, 11), MP.init_params(cfg_p, 11)
    for w, g_ in zip(want, got):
        assert list(w) == list(g_)
        for k in w:
            assert np.array_equal(np.asarray(w[k]).view(np.uint32), np.asarray(g_[k]).view(np.uint32)), k
    b = AH.batch_to_torch(AH.synth_batch(cfg_s, B, seed=3), torch.float64)
    noise = O.noise_to_torch(O.make_noise(cfg_s, B, seed=7, utd_ratio=2), torch.float64)
    with MS.installed():
        st0 = O.TrainState(cfg_s, *want, torch.float64)
        info0, aux0 = O.update_high_utd(st0, b, noise, 2)
    with MP.installed():
        assert O.critic_forward is MP.critic_forward
        st1 = O.TrainState(cfg_p, *got, torch.float64)
        info1, aux1 = O.update_high_utd(st1, b, noise, 2)
    assert O.critic_forward is not MP.critic_forward and O.init_params is not MP.init_params
    assert info0 == info1
    for k, v in aux0["g_actor"].items():
        assert torch.equal(v, aux1["g_actor"][k]), k
    for sec, tree in _oracle_sections(st0).items():
        for leaf, t in tree.items():
            assert torch.equal(t, _oracle_sections(st1)[sec][leaf]), (sec, leaf)


# ---- the reference's own tree, initial parameters and update code -----------------------------------------------------------------
class _PlainCore:
    """what export_tree reads of a core: cfg, the two lists, the two flags, and get(section, leaf) -> the leaf's flat values"""

    def __init__(self, cfg):
        self.cfg = SimpleNamespace(n_cam=cfg.n_cam, H=cfg.H, W=cfg.W, state_dim=cfg.S, act_dim=cfg.A, ensemble=cfg.ensemble,
                                   hidden=cfg.hidden, encoder_type=1 if cfg.encoder_type == "small" else 0, num_stack=1)
        self.critic_dims, self.policy_dims = cfg.critic_dims, cfg.policy_dims
        self.critic_layer_norm, self.policy_layer_norm = cfg.critic_layer_norm, cfg.policy_layer_norm
        self.shapes = dict(pinit.theta_shapes(cfg.n_cam, cfg.H, cfg.W, cfg.S, cfg.A, ensemble=cfg.ensemble, encoder_type=cfg.encoder_type,
                                              critic_dims=cfg.critic_dims, policy_dims=cfg.policy_dims,
                                              critic_layer_norm=cfg.critic_layer_norm, policy_layer_norm=cfg.policy_layer_norm),
                           **FT.trunk_shapes())

    def get(self, section, leaf):
        return np.zeros(int(np.prod(self.shapes[leaf])), np.float32)


def _goldens():
    out = [(f"update_{n}", MP.load_golden(n)) for n in MP.UPDATE_GOLDEN]
    z, cfg, _, _ = MP.init_golden()
    g = G.unpack(z)
    g["cfg"] = cfg
    return out + [("init_sac_state", g)]


@pytest.mark.parametrize("name,g", _goldens(), ids=[n for n, _ in _goldens()])
def test_shapes_paths_and_export_are_the_references_tree(name, g):
    cfg, want = g["cfg"], g["meta"]["param_tree"]
    assert g["meta"]["mlp_plain"] == MP.meta_of(cfg) and not (cfg.critic_layer_norm and cfg.policy_layer_norm)
    kw = dict(critic_dims=cfg.critic_dims, policy_dims=cfg.policy_dims, critic_layer_norm=cfg.critic_layer_norm,
              policy_layer_norm=cfg.policy_layer_norm)
    shapes = pinit.theta_shapes(cfg.n_cam, cfg.H, cfg.W, cfg.S, cfg.A, ensemble=cfg.ensemble, encoder_type=cfg.encoder_type, **kw)
    paths = FT.theta_paths(cfg.image_keys, encoder_type=cfg.encoder_type, **kw)
    assert list(paths) and set(paths) == set(shapes)
    assert [AH.product_name(k, cfg.image_keys) for k in MP.trainable_param_shapes(cfg)] == list(shapes)     # arena order
    for net, dims, ln in (("modules_critic", cfg.critic_dims, cfg.critic_layer_norm), ("modules_actor", cfg.policy_dims, cfg.policy_layer_norm)):
        mods = want[net]["network"]      # the reference's own tree: no LayerNorm_* under a plain network
        assert sorted(mods) == sorted([f"Dense_{j}" for j in range(len(dims))] + ([f"LayerNorm_{j}" for j in range(len(dims))] if ln else []))
    assert G.shape_tree(FT.export_tree(_PlainCore(cfg), "params", cfg.image_keys)) == want


def test_host_twins_equal_the_reference_initial_params_without_the_layer_norm_leaves():
    z, cfg, recs, shapes = MP.init_golden()
    assert cfg.critic_dims == (128, 64) and cfg.policy_dims == (64, 64, 128) and (cfg.critic_layer_norm, cfg.policy_layer_norm) == (True, False)
    assert not any(k.startswith("actor/ln") for k in recs) and "critic/ln2/scale" in recs
    got = IR.theta_reference(cfg.image_keys, cfg.H, cfg.W, cfg.S, cfg.A, 0, ensemble=cfg.ensemble, encoder_type=cfg.encoder_type,
                             temperature_init=1e-2, device=None, critic_dims=cfg.critic_dims, policy_dims=cfg.policy_dims,
                             critic_layer_norm=cfg.critic_layer_norm, policy_layer_norm=cfg.policy_layer_norm)
    assert set(got) == set(recs), sorted(set(got) ^ set(recs))
    bad = [m for m in (IG.mismatch(n, recs[n], got[n]) for n in sorted(recs)) if m]
    assert not bad, bad
    for n, v in got.items():
        assert tuple(v.shape) == shapes[n], (n, v.shape, shapes[n])
    assert np.array_equal(IR.create_rng_of(0), z["init_rng"])      # state.rng after create does not depend on the flags


@pytest.mark.parametrize("name", MP.UPDATE_GOLDEN)
def test_general_oracle_reproduces_the_reference_golden(name):
    g = MP.load_golden(name)
    cfg = g["cfg"]
    with MP.installed():
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
    print(f"plain_update_{name}: general oracle vs reference golden, worst {worst:.1e}")


# ---- the relu cases of the GPU table stay clear of the kink -----------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in MP.CASES if "relu" in (c[9], c[10])], ids=[c[0] for c in MP.CASES if "relu" in (c[9], c[10])])
def test_relu_pre_activations_of_the_gpu_cases_stay_clear_of_zero(case):
    assert case[1] == "state"        # (a pixel case would run the fp64 trunk here)
    with MP.installed():
        worst = MP.check_relu_margin(case)
    print(f"{case[0]}: min |relu pre-activation| over the case's oracle runs {worst:.3g}")
    assert worst >= MP.RELU_MARGIN
