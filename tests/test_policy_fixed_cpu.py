"""CPU: the policy head with a fixed standard deviation (policy_fixed=True; std_parameterization="fixed" with fixed_std,
actor_critic_nets.py:189-192,212; tests/policy_fixed.py).

* utils.init.policy_mode_fixed: what it returns, every refusal from the arguments alone, a scalar against the vector of it; without
  the switch the old refusals stand; Dropout beside a fixed head is refused naming both switches;
* theta_shapes, flax_tree.theta_paths, init_theta and init_ref's host twins hold no std leaf, and the shared leaves are those of the
  "exp" tree bit for bit;
* both checkpoint refusals, on host trees;
* the C ABI as far as no device is needed: the header declares the new symbols, the library exports them, the bindings cover
  them, and serl_agent_create_fixed_std's three argument errors;
* the fp64 statement (the oracle in "uniform" with actor/log_stds pinned): its std equals clip(fixed_std) to 1e-15 in every policy
  evaluation of every case, its own log_stds gradient is not zero there, and it reproduces the reference's own update code on
  tests/golden/fixed_*.npz within the F64_TOL of tests/test_reference_update.py."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import drq_oracle as O
from oracle import golden_update as G
from oracle import ref_update_runner as RR
import agent_helpers as AH
import policy_fixed as PF
import policy_modes as PM
from serl_amd.agents import flax_tree as FT
from serl_amd.utils import init as pinit
from serl_amd.utils import init_ref as IR
from test_mlp_widths_cpu import _create_drq, _create_states
from test_reference_update import F64_TOL, _oracle_sections

CREATE = pytest.mark.parametrize("create", [_create_states, _create_drq], ids=["create_states", "create_drq"])
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pk(**kw):
    return {"tanh_squash_distribution": True, "std_min": 1e-5, "std_max": 5, **kw}


# ---- the argument reader ---------------------------------------------------------------------------------------------------------
def test_policy_mode_fixed_returns_the_mode_and_a_float32_vector():
    std, squash, fixed = pinit.policy_mode_fixed(_pk(std_parameterization="fixed", fixed_std=0.1), 5)
    assert (std, squash) == ("fixed", True) and fixed.dtype == np.float32 and fixed.shape == (5,) and fixed.flags.writeable
    assert np.array_equal(fixed, np.full(5, np.float32(0.1)))
    vec = [0.01, 0.3, 1.0, 5.0, 0.7]
    std, squash, fixed = pinit.policy_mode_fixed(_pk(std_parameterization="fixed", fixed_std=vec, tanh_squash_distribution=False), 5)
    assert (std, squash) == ("fixed", False) and np.array_equal(fixed, np.asarray(vec, np.float32))
    # a scalar is the vector of it, in every form a caller may write one
    want = pinit.policy_mode_fixed(_pk(std_parameterization="fixed", fixed_std=[0.1] * 3), 3)[2]
    for scalar in (0.1, np.float32(0.1), np.float64(0.1), [0.1], np.array(0.1), np.array([0.1])):
        got = pinit.policy_mode_fixed(_pk(std_parameterization="fixed", fixed_std=scalar), 3)[2]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), scalar
    assert np.array_equal(pinit.policy_mode_fixed(_pk(std_parameterization="fixed", fixed_std=2), 1)[2], np.ones(1, np.float32) * 2)


def test_any_other_mode_under_the_switch_is_read_as_without_it():
    for pk in (None, {}, PM.policy_kwargs("uniform", False), PM.policy_kwargs("softplus", True), PM.policy_kwargs("exp", True)):
        assert pinit.policy_mode_fixed(pk, 4) == (*pinit.policy_mode(pk), None)
    with pytest.raises(NotImplementedError, match="std_parameterization='tanh'"):
        pinit.policy_mode_fixed({"std_parameterization": "tanh"}, 4)


def test_every_refusal_comes_from_the_arguments_alone():
    with pytest.raises(ValueError, match="Invalid std_parameterization"):
        pinit.policy_mode_fixed({"std_parameterization": "fixed"}, 4)                     # as the reference raises
    with pytest.raises(ValueError, match="Invalid std_parameterization"):
        pinit.policy_mode_fixed({"std_parameterization": "fixed", "fixed_std": None}, 4)
    for std in ("exp", "softplus", "uniform"):
        with pytest.raises(NotImplementedError, match=f"fixed_std.* with std_parameterization='{std}'"):
            pinit.policy_mode_fixed({"std_parameterization": std, "fixed_std": 0.1}, 4)
    with pytest.raises(NotImplementedError, match="fixed_std.* with std_parameterization='exp'"):
        pinit.policy_mode_fixed({"fixed_std": [0.1] * 4}, 4)                               # absent: the launcher's "exp"
    for bad in ([0.1, 0.2], [0.1] * 5, [], [[0.1] * 4]):
        with pytest.raises(ValueError, match="fixed_std.* has shape"):
            pinit.policy_mode_fixed({"std_parameterization": "fixed", "fixed_std": bad}, 4)
    for bad in (0.0, -0.1, float("nan"), float("inf"), [0.1, 0.2, 0.0, 0.3], [0.1, float("nan"), 0.1, 0.1], 1e-60, 1e60):
        with pytest.raises(ValueError, match="finite positive"):
            pinit.policy_mode_fixed({"std_parameterization": "fixed", "fixed_std": bad}, 4)     # (1e-60 and 1e60 as float32: 0 and inf)
    with pytest.raises(ValueError, match="is not a number"):
        pinit.policy_mode_fixed({"std_parameterization": "fixed", "fixed_std": "wide"}, 4)


@CREATE
def test_create_refuses_from_the_arguments_alone(create):
    """no device is touched: this test runs without one"""
    with pytest.raises(ValueError, match="Invalid std_parameterization"):
        create(policy_kwargs=_pk(std_parameterization="fixed"), policy_fixed=True)
    with pytest.raises(NotImplementedError, match="with std_parameterization='uniform'"):
        create(policy_kwargs=_pk(std_parameterization="uniform", fixed_std=0.1), policy_fixed=True)
    with pytest.raises(ValueError, match="has shape"):
        create(policy_kwargs=_pk(std_parameterization="fixed", fixed_std=[0.1, 0.2]), policy_fixed=True)
    with pytest.raises(ValueError, match="finite positive"):
        create(policy_kwargs=_pk(std_parameterization="fixed", fixed_std=-1.0), policy_fixed=True)


@CREATE
def test_without_the_switch_the_old_refusals_stand(create):
    for extra in ({}, {"policy_fixed": False}):
        with pytest.raises(NotImplementedError, match="std_parameterization='fixed'"):
            create(policy_kwargs=_pk(std_parameterization="fixed", fixed_std=0.1), **extra)
        with pytest.raises(NotImplementedError, match="fixed_std"):
            create(policy_kwargs=_pk(fixed_std=0.1), **extra)


@CREATE
def test_dropout_beside_a_fixed_head_is_refused_naming_both_switches(create):
    for ck, pk in (({"dropout_rate": 0.1}, {}), ({}, {"dropout_rate": 0.2})):
        with pytest.raises(NotImplementedError, match="std_parameterization='fixed'") as e:
            create(policy_kwargs=_pk(std_parameterization="fixed", fixed_std=0.1), policy_fixed=True, mlp_dropout=True,
                   critic_network_kwargs=ck, policy_network_kwargs=pk)
        assert "policy_fixed=True" in str(e.value) and "mlp_dropout=True" in str(e.value)
    pinit.NetSpec(critic_dropout=0.1, policy_dropout=0.2).check()                              # no fixed head: Dropout's own business
    pinit.NetSpec(std_parameterization="fixed", fixed_std=(1.0, 1.0, 1.0)).check()             # no positive rate: served


# ---- shapes and trees ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cam,H,W,etype", [(0, 0, 0, "resnet-pretrained"), (2, 64, 64, "resnet-pretrained"), (1, 64, 64, "small")])
@pytest.mark.parametrize("kw", [{}, {"critic_dims": (320,), "policy_dims": (64, 128), "critic_layer_norm": False}], ids=["256x256", "shapes_plain"])
def test_no_std_leaf_and_the_shared_leaves_of_the_exp_tree(n_cam, H, W, etype, kw):
    keys = ("front", "wrist")[:n_cam]
    S, A = 7, 3
    exp = pinit.theta_shapes(n_cam, H, W, S, A, ensemble=3, encoder_type=etype, **kw)
    got = pinit.theta_shapes(n_cam, H, W, S, A, ensemble=3, encoder_type=etype, std_parameterization="fixed", **kw)
    assert list(got.items()) == [(k, v) for k, v in exp.items() if k not in PM.STD_DENSE]      # the others, in the arena's order
    assert not any("logstd" in k or "log_stds" in k for k in got) and list(got)[-2:] == ["actor/mean/bias", "temp/lagrange"]
    assert pinit._policy_std_shapes(64, A, "fixed") == {}
    paths, exp_paths = FT.theta_paths(keys, encoder_type=etype, std_parameterization="fixed", **kw), FT.theta_paths(keys, encoder_type=etype, **kw)
    assert set(paths) == set(got) and all(paths[k] == exp_paths[k] for k in paths)
    assert not any(p[0][:2] in (("modules_actor", "Dense_1"), ("modules_actor", "log_stds")) for p in paths.values())
    a = pinit.init_theta(n_cam, H, W, S, A, seed=5, ensemble=3, encoder_type=etype, **kw)
    b = pinit.init_theta(n_cam, H, W, S, A, seed=5, ensemble=3, encoder_type=etype, std_parameterization="fixed", **kw)
    assert list(b) == list(got)
    # (the numpy stream draws leaf by leaf in arena order: the std Dense stands behind every shared actor leaf but the temperature,
    #  which is no draw)
    for k in b:
        assert np.array_equal(np.asarray(a[k]).view(np.uint32), np.asarray(b[k]).view(np.uint32)), k
    if n_cam < 2:
        ra = IR.theta_reference(keys, H, W, S, A, 0, ensemble=3, encoder_type=etype, device=None, **kw)
        rb = IR.theta_reference(keys, H, W, S, A, 0, ensemble=3, encoder_type=etype, device=None, std_parameterization="fixed", **kw)
        assert list(rb) == list(got) and set(ra) - set(rb) == set(PM.STD_DENSE)
        for k in rb:       # flax keys depend on a module's own path: dropping Dense_1 moves no other leaf, as for "uniform"
            assert np.array_equal(ra[k].view(np.uint32), rb[k].view(np.uint32)), k


def test_the_test_side_leaf_table_is_the_librarys():
    for name in PF.IDS:
        cfg, _, _ = PF.case_config(name)
        cln, pln = cfg.critic_layer_norm, cfg.policy_layer_norm
        shapes = pinit.theta_shapes(cfg.n_cam, cfg.H, cfg.W, cfg.S, cfg.A, ensemble=cfg.ensemble, encoder_type=cfg.encoder_type,
                                    std_parameterization="fixed", critic_dims=cfg.critic_dims, policy_dims=cfg.policy_dims,
                                    critic_layer_norm=cln, policy_layer_norm=pln)
        mine = PF.trainable_param_shapes(cfg)
        assert [AH.product_name(k, cfg.image_keys) for k in mine] == list(shapes)
        pinned = PF.trainable_param_shapes(PF.pinned_config(cfg))
        assert [k for k in pinned if k != PF.LEAF] == list(mine) and pinned[PF.LEAF] == (cfg.A,)
        trunk, theta = PF.init_params(cfg, 3)
        pt = PF.pinned_theta(cfg, theta)
        assert list(pt) == list(pinned) and pt[PF.LEAF].dtype == np.float64
        assert np.array_equal(np.exp(pt[PF.LEAF]).round(12), PF.clip_fixed(cfg).round(12))


# ---- checkpoints: both refusals ------------------------------------------------------------------------------------------------------
class _Core:
    """what load_state_dict reads of a core: cfg.encoder_type, the mode, the leaf counts and set()"""

    def __init__(self, std, A=3, S=7):
        self.cfg = SimpleNamespace(encoder_type=0, hidden=64)
        self.std_parameterization = std
        self.shapes = pinit.theta_shapes(0, 0, 0, S, A, ensemble=2, hidden=64, std_parameterization=std)
        self.leaves = {k: int(np.prod(v)) if len(v) else 1 for k, v in self.shapes.items()}
        self.written, self.step = [], 0

    def set(self, section, leaf, v):
        self.written.append((section, leaf))

    def get(self, section, leaf):
        return np.zeros(self.leaves[leaf], np.float32)


def _agent(std):
    core = _Core(std)
    core.cfg.n_cam, core.cfg.H, core.cfg.W, core.cfg.state_dim, core.cfg.act_dim, core.cfg.ensemble, core.cfg.num_stack = 0, 0, 0, 7, 3, 2, 1
    return SimpleNamespace(core=core, image_keys=())


def _tree_of(std):
    return FT.export_tree(_agent(std).core, "params", ())


@pytest.mark.parametrize("other", ["exp", "softplus", "uniform"])
def test_checkpoint_refusals_between_fixed_and_std_leaves(other):
    from serl_amd.utils.checkpoint import load_state_dict
    fixed_tree, other_tree = _tree_of("fixed"), _tree_of(other)
    assert "Dense_1" not in fixed_tree["modules_actor"] and "log_stds" not in fixed_tree["modules_actor"]
    held = "log_stds" if other == "uniform" else "Dense_1"
    assert held in other_tree["modules_actor"]
    fixed = _agent("fixed")
    for sd in ({"params": other_tree}, {"target_params": other_tree}, {"params": fixed_tree, "target_params": other_tree}):
        with pytest.raises(ValueError, match=rf"the state holds the policy's std leaves \('modules_actor/{held}'\), this agent's head has a fixed "
                                             r"std and no std leaf .*nothing was loaded"):
            load_state_dict(fixed, sd)
    agent = _agent(other)
    with pytest.raises(ValueError, match=r"the state holds no std leaf of the policy .*std_parameterization='fixed' agent.*nothing was loaded"):
        load_state_dict(agent, {"params": other_tree, "target_params": fixed_tree})
    assert fixed.core.written == [] and agent.core.written == []
    # ... and each loads its own kind
    load_state_dict(fixed, {"params": fixed_tree})
    load_state_dict(agent, {"params": other_tree})
    assert len(fixed.core.written) == len(fixed.core.leaves) and len(agent.core.written) == len(agent.core.leaves)


# ---- the C ABI, as far as no device is needed ------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    from serl_amd import _lib, _lib_agent
    L = _lib.lib()
    decl = _lib.exported_symbols()
    for name, nargs in (("serl_agent_create_fixed_std", 13), ("serl_agent_fixed_std", 2)):
        assert hasattr(L, name) and name in decl and name in _lib_agent.SIGNATURES, name
        assert decl[name] == len(_lib_agent.SIGNATURES[name]) == nargs, name
    header = open(os.path.join(ROOT, "include", "serl_mi355.h")).read()
    assert re.search(r"#define SERL_STD_FIXED 3\b", header)
    assert len(_lib_agent.SIGNATURES["serl_agent_create_fixed_std"]) == len(_lib_agent.SIGNATURES["serl_agent_create_layer_norm"]) + 1
    assert _lib_agent.SerlAgentCfg._fields_[-1][0] == "num_stack"       # the struct is the one it was
    assert pinit.STD_PARAMETERIZATIONS == ("exp", "softplus", "uniform") and pinit.FIXED_STD == "fixed"


def test_create_fixed_std_argument_errors():
    """the pointer is NULL unless std_param == SERL_STD_FIXED, and the entries are finite and positive: refused before any device call"""
    from serl_amd import _lib
    from serl_amd._lib_agent import SerlAgentCfg
    SERL_ERR_INVALID, SERL_STD_FIXED = -1, 3      # include/serl_mi355.h
    L = _lib.lib()
    cfg = SerlAgentCfg(0, 0, 0, 0, 10, 4, 8, 10, 256, 256, 8, 64, 0, -1, 0.99, 0.005, 3e-4, 0.1, 1e-5, 5.0, -2.0, 0)
    dims = (C.c_int32 * 2)(64, 128)

    def create(std_param, fixed):
        h = C.c_void_p()
        fs = None if fixed is None else (C.c_float * 4)(*fixed)
        rc = int(L.serl_agent_create_fixed_std(C.byref(cfg), std_param, 0, 0, 0, dims, 2, dims, 1, 1, 1, fs, C.byref(h)))
        return rc, (L.serl_last_error() or b"").decode(), h
    for std_param, fixed, what in ((SERL_STD_FIXED, None, "needs fixed_std"), (0, [0.1] * 4, "fixed_std is given with std_param 0"),
                                   (2, [0.1] * 4, "fixed_std is given with std_param 2"), (SERL_STD_FIXED, [0.1, 0.0, 0.1, 0.1], "fixed_std[1]"),
                                   (SERL_STD_FIXED, [0.1, 0.1, 0.1, float("nan")], "fixed_std[3]"), (SERL_STD_FIXED, [-1.0] * 4, "fixed_std[0]"),
                                   (4, None, "std_param 4"), (-1, None, "std_param -1")):
        rc, msg, h = create(std_param, fixed)
        assert rc == SERL_ERR_INVALID and what in msg and not h.value, (std_param, fixed, rc, msg)
    # serl_agent_create_layer_norm keeps refusing 3 by its own range check, with the message it always gave
    h = C.c_void_p()
    rc = int(L.serl_agent_create_layer_norm(C.byref(cfg), SERL_STD_FIXED, 0, 0, 0, dims, 2, dims, 1, 1, 1, C.byref(h)))
    msg = (L.serl_last_error() or b"").decode()
    assert rc == SERL_ERR_INVALID and "std_param 3 is not SERL_STD_EXP (0), SERL_STD_SOFTPLUS (1) or SERL_STD_UNIFORM (2)" in msg, (rc, msg)
    out = (C.c_float * 4)()
    assert int(L.serl_agent_fixed_std(None, out)) == SERL_ERR_INVALID


def test_golden_files_stay_out_of_the_update_sweeps_and_under_the_size_limit():
    for name in PF.GOLDEN:
        path = PF.golden_path(name)
        assert os.path.basename(path).startswith("fixed_") and os.path.getsize(path) < 1 << 20


# ---- the fp64 statement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in PF.IDS if PF.CASES[n]["kind"] == "state"])
def test_pinned_oracle_has_the_fixed_std_and_a_log_stds_gradient_of_its_own(name):
    """(the pixel cases run the same code behind an fp64 trunk pass; the GPU tests assert their records)"""
    cfg, B, utd = PF.case_config(name)
    want = PF.clip_fixed(cfg)
    with PF.installed():
        for call in PF.calls_of(name):
            run = PF.oracle_run(name, call)
            pin, st = run["pin"], run["state"]
            n_crit = 1 if call == "critics" else call[1]
            assert pin["evaluations"] == n_crit + (0 if call == "critics" else 2) and pin["steps"] == n_crit + (0 if call == "critics" else 1)
            assert pin["std_err"] <= PF.STD_TOL, (name, call, pin)
            # the leaf is back where it was pinned after every step, whatever its gradient and its moments did
            assert np.allclose(np.exp(st.params[PF.LEAF].numpy()), want, rtol=0, atol=1e-15)
            if call != "critics":
                g = run["aux"]["g_actor"][PF.LEAF].numpy()
                assert g.shape == (cfg.A,) and np.abs(g).min() > 0, (name, call, g)     # a uniform agent would move log_stds
                inside = (np.asarray(cfg.fixed_std) > cfg.std_min) & (np.asarray(cfg.fixed_std) < cfg.std_max)
                assert (st.opt["actor"]["mu"][PF.LEAF].numpy()[inside] != 0).all()
                assert set(run["aux"]["g_actor"]) - {PF.LEAF} == {k for k in PF.trainable_param_shapes(cfg) if k.startswith("actor/")}
    if name.startswith("a_"):
        assert want.tolist() == [0.05, float(np.float32(0.3)), 1.0, 2.0, float(np.float32(0.7))]       # two columns clipped


def _pinned_replay(name):
    g, meta, z = PF.load_golden(name)
    cfg = g["cfg"]
    trunk, theta = PF.initial_leaves(cfg)
    st = PF.pinned_state(cfg, trunk, theta)
    worst_i = 0.0

    def check(i, step, info):
        nonlocal worst_i
        assert set(info) == {k for k in step["info"] if not k.endswith("_lr")}
        for k, v in info.items():
            r = step["info"][k]
            worst_i = max(worst_i, abs(v - r) / max(1.0, abs(r)))
            assert abs(v - r) <= F64_TOL * max(1.0, abs(r)), (i, k, v, r)
    with PF.pinned(cfg) as pin:
        RR.run_steps(st, g["steps"], torch.float64, on_info=check)
    return g, meta, z, st, pin, worst_i


@pytest.mark.parametrize("name", list(PF.GOLDEN))
def test_pinned_oracle_reproduces_the_reference_golden(name):
    """tests/test_reference_update.py::test_oracle_reproduces_the_reference_golden on fixed_<name>.npz: the reference's own update
    code with std_parameterization="fixed" against the pinned oracle -- every info scalar and the whole final state, the pinned
    leaf left out (the reference has no such leaf), within F64_TOL"""
    with PF.installed():
        g, meta, z, st, pin, worst_i = _pinned_replay(name)
        cfg = g["cfg"]
        pf = meta["policy_fixed"]
        assert pf["fixed_std"] == list(cfg.fixed_std) and pf["tanh_squash_distribution"] == cfg.tanh_squash
        assert (pf["std_min"], pf["std_max"], pf["backup_entropy"]) == (cfg.std_min, cfg.std_max, cfg.backup_entropy)
        actor = meta["param_tree"]["modules_actor"]
        assert "Dense_1" not in actor and "log_stds" not in actor and "Dense_0" in actor      # the reference's own tree
        # the stddev of every distribution the reference built is clip(fixed_std), and the oracle evaluated as many
        assert z["fixed_stddev"].shape == (pf["policy_evaluations"], cfg.A) == (pin["evaluations"], cfg.A)
        assert np.array_equal(z["fixed_stddev"], np.broadcast_to(PF.clip_fixed(cfg), z["fixed_stddev"].shape))
        assert pin["std_err"] <= PF.STD_TOL and st.step == meta["final_step"]
        stored = {k[2:].split("|")[1] for k in z.files if k.startswith("f_params|")}
        assert stored == set(O.trainable_param_shapes(cfg)) and PF.LEAF not in stored
        worst = 0.0
        for sec, tree in _oracle_sections(st).items():
            tree = PF.unpinned(tree)
            assert set(g["final"][sec]) == set(tree), sec
            for leaf, t in tree.items():
                e, how = G.leaf_compare(f"{sec}/{leaf}", g["final"][sec][leaf], t.numpy())
                assert e < F64_TOL, (sec, leaf, how, e)
                worst = max(worst, e)
    print(f"fixed_{name}: pinned oracle vs reference golden, infos {worst_i:.1e}, final state {worst:.1e}")


def test_flax_paths_of_a_fixed_agent_equal_the_recorded_tree():
    for name in PF.GOLDEN:
        g, meta, _ = PF.load_golden(name)
        cfg = g["cfg"]
        paths = FT.theta_paths(cfg.image_keys, encoder_type=cfg.encoder_type, std_parameterization="fixed")
        shapes = pinit.theta_shapes(cfg.n_cam, cfg.H, cfg.W, cfg.S, cfg.A, ensemble=cfg.ensemble, hidden=cfg.hidden,
                                    encoder_type=cfg.encoder_type, std_parameterization="fixed")

        def leaf_paths(tree, prefix=()):
            for k, v in tree.items():
                if isinstance(v, dict):
                    yield from leaf_paths(v, prefix + (k,))
                else:
                    yield prefix + (k,), tuple(v)
        want = {p: s for p, s in leaf_paths(meta["param_tree"]) if "pretrained_encoder" not in p}
        assert {ps[0]: tuple(shapes[leaf]) for leaf, ps in paths.items()} == want
