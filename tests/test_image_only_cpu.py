"""CPU: agents without the proprio branch (create_drq(image_only=True, use_proprio=False); serl_agent_opts.no_proprio): the refusals
on both sides of the C ABI, NetSpec's round trip, the leaf tables and the flax tree of an image-only agent, the general oracle of
tests/image_only.py with use_proprio=True against tests/policy_fixed.py's bit for bit, and the conditioning of the frame-stack case.

Every test but the pinned refusal fails on a tree without the option: create_drq, NetSpec and SerlAgentOpts do not know it."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from oracle import drq_oracle as O
import agent_helpers as AH
import image_only as IO
import policy_fixed as PF
from serl_amd.utils import init as pinit
from serl_amd.utils.init import NetSpec
from test_agent_opts_cpu import SERL_ERR_INVALID, _cfg, _create

SERL_ERR_UNSUPPORTED = -4      # include/serl_mi355.h
OBS = {"wrist": np.zeros((32, 32, 3), np.uint8), "state": np.zeros((5,), np.float32)}
ACT = np.zeros((3,), np.float32)


def _drq(**kw):
    from serl_amd.agents.drq import DrQAgent
    return DrQAgent.create_drq(0, OBS, ACT, encoder_type="small", image_keys=("wrist",), **kw)


# ---- Python: what the arguments alone decide ----------------------------------------------------------------------------------------
def test_without_the_switch_the_refusal_is_the_pinned_one_and_names_the_switch():
    with pytest.raises(NotImplementedError, match="only use_proprio=True") as e:
        _drq(use_proprio=False)
    assert "image_only=True" in str(e.value)
    with pytest.raises(NotImplementedError, match="only use_proprio=True"):
        _drq()          # the reference's own default


@pytest.mark.parametrize("bad", [None, 0, 1, "False", 0.0, np.zeros(1)])
def test_a_use_proprio_that_is_no_bool_is_refused_under_the_switch(bad):
    with pytest.raises(NotImplementedError, match=r"use_proprio=.* under image_only=True \(served: True or False\)"):
        _drq(use_proprio=bad, image_only=True)


def test_dropout_beside_image_only_is_refused_naming_both_switches():
    kw = {"activations": "tanh", "use_layer_norm": True, "hidden_dims": [256, 256], "dropout_rate": 0.1}
    with pytest.raises(NotImplementedError) as e:
        _drq(use_proprio=False, image_only=True, mlp_dropout=True, critic_network_kwargs=kw)
    assert "image_only=True" in str(e.value) and "mlp_dropout=True" in str(e.value)
    with pytest.raises(NotImplementedError, match="image_only=True"):
        NetSpec(critic_dropout=0.1, use_proprio=False).check()
    assert NetSpec(critic_dropout=0.1).check().critic_dropout == 0.1      # with the proprio branch: served as always
    assert NetSpec(use_proprio=False).check().use_proprio is False


def test_the_trunk_farm_refuses_an_image_only_core():
    from serl_amd.parallel import TrunkFarmLearner

    class Core:
        live_trunk, use_proprio = False, False
    with pytest.raises(NotImplementedError, match="image-only"):
        TrunkFarmLearner(Core(), None, [], [])


def test_the_spec_of_a_call_carries_the_flag(monkeypatch):
    """create_drq hands AgentCore the NetSpec of its arguments; no core is made"""
    import serl_amd.agents.drq as drq

    class Stop(Exception):
        pass
    seen = []

    def no_core(**k):
        seen.append(NetSpec(**{f.name: k[f.name] for f in dataclasses.fields(NetSpec)}))
        raise Stop
    monkeypatch.setattr(drq, "AgentCore", no_core)
    for kw in (dict(use_proprio=False, image_only=True), dict(use_proprio=True, image_only=True), dict(use_proprio=True)):
        with pytest.raises(Stop):
            _drq(**kw)
    assert seen == [NetSpec(use_proprio=False), NetSpec(), NetSpec()]


# ---- NetSpec and the C struct ------------------------------------------------------------------------------------------------------
def test_netspec_round_trip_and_the_all_zero_struct():
    from serl_amd import _lib_agent
    from serl_amd.utils.launcher import make_drq_agent  # noqa: F401  (the launcher's agent is the default NetSpec)
    spec = NetSpec(use_proprio=False)
    o = spec.to_c()
    assert o.no_proprio == 1 and NetSpec().to_c().no_proprio == 0
    assert bytes(NetSpec().to_c()) == bytes(_lib_agent.SerlAgentOpts())          # all zero: serl_agent_create(cfg)
    assert _lib_agent.SerlAgentOpts._fields_[-1] == ("no_proprio", C.c_int)
    assert _lib_agent.SerlAgentCfg._fields_[-1] == ("num_stack", C.c_int)          # serl_agent_cfg is the struct it was
    assert spec.core_kwargs()["use_proprio"] is False and NetSpec().core_kwargs()["use_proprio"] is True
    assert spec.leaf_kwargs()["use_proprio"] is False and "use_proprio" not in NetSpec().leaf_kwargs()
    assert spec.config_entries()["use_proprio"] is False and "use_proprio" not in NetSpec().config_entries()
    assert dataclasses.replace(spec, use_proprio=True) == NetSpec()


def _pixel_cfg(n_cam=1):
    from serl_amd._lib_agent import SerlAgentCfg
    return SerlAgentCfg(0, n_cam, 32, 32, 5, 3, 6, 2, 256, 256, 8, 64, 0, -1, 0.96, 0.005, 3e-4, 0.1, 1e-5, 5.0, -1.5, 0)


def test_c_refusals():
    rc, msg = _create(NetSpec(use_proprio=False).to_c())            # test_agent_opts_cpu._cfg: a state-only agent
    assert rc == SERL_ERR_INVALID and "no_proprio 1 with n_cam 0" in msg, msg
    for value in (2, -1, 64):
        o = NetSpec().to_c()
        o.no_proprio = value
        for cfg in (_cfg(), _pixel_cfg()):
            rc, msg = _create(o, cfg)
            assert rc == SERL_ERR_INVALID and f"no_proprio {value} is not" in msg, msg
    o = NetSpec(use_proprio=False).to_c()
    o.policy.dropout = 0.25
    rc, msg = _create(o, _pixel_cfg())
    assert rc == SERL_ERR_UNSUPPORTED and "no_proprio 1" in msg and "dropout 0 / 0.25" in msg, msg
    rc, msg = _create(NetSpec(use_proprio=False).to_c(), _pixel_cfg())
    assert rc not in (SERL_ERR_INVALID, SERL_ERR_UNSUPPORTED), msg      # (made and destroyed where a device is present)
    from serl_amd import _lib
    assert int(_lib.lib().serl_agent_use_proprio(None)) == -1


# ---- leaf tables and the flax tree ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("encoder_type,keys", [("resnet-pretrained", ("wrist",)), ("small", ("wrist", "front"))])
def test_leaf_tables_of_an_image_only_agent(encoder_type, keys):
    from serl_amd.agents.flax_tree import theta_paths
    from serl_amd.utils.init_ref import theta_leaves
    n, A, N = len(keys), 3, 10
    kw = NetSpec(use_proprio=False).leaf_kwargs()
    sh = pinit.theta_shapes(n, 64, 64, 5, A, ensemble=N, encoder_type=encoder_type, **kw)
    full = pinit.theta_shapes(n, 64, 64, 5, A, ensemble=N, encoder_type=encoder_type)
    assert not any(k.startswith("enc/proprio") for k in sh) and set(full) - set(sh) == {k for k in full if k.startswith("enc/proprio")}
    assert sh["critic/w1"] == (N, 256 * n + A, 256) and sh["actor/w1"] == (256 * n, 256)
    assert {k: v for k, v in sh.items() if k not in ("critic/w1", "actor/w1")} == {k: full[k] for k in sh if k not in ("critic/w1", "actor/w1")}
    assert list(sh) == [k for k in full if not k.startswith("enc/proprio")]          # the arena's order
    paths = theta_paths(keys, encoder_type=encoder_type, **kw)
    assert set(paths) == set(sh)
    enc = [p[0] for p in paths.values() if p[0][:2] == ("modules_actor", "encoder")]
    assert enc and all(p[2].startswith("encoder_") for p in enc)                        # no Dense_0 / LayerNorm_0 under `encoder`
    assert [lf.name for lf in theta_leaves(keys, 64, 64, 5, A, ensemble=N, encoder_type=encoder_type, **kw)] == list(sh)
    # the oracle's leaf table is the same one, oracle names
    with IO.installed():
        cfg = IO.ImageOnlyConfig(image_keys=keys, H=64, W=64, S=5, A=A, ensemble=N, encoder_type=encoder_type, use_proprio=False)
        osh = {AH.product_name(k, keys): tuple(v) for k, v in O.trainable_param_shapes(cfg).items()}
    assert osh == {k: tuple(v) for k, v in sh.items()} and list(osh) == list(sh)


def test_init_theta_keeps_the_shared_leaves_of_the_proprio_agent_of_the_same_seed():
    a = pinit.init_theta(2, 64, 64, 5, 3, seed=9, ensemble=2, use_proprio=False)
    b = pinit.init_theta(2, 64, 64, 5, 3, seed=9, ensemble=2)
    assert list(a) == [k for k in b if not k.startswith("enc/proprio")]
    for k, v in a.items():
        if k in ("critic/w1", "actor/w1"):
            fan = v.shape[-2] + v.shape[-1]
            assert v.dtype == np.float32 and np.abs(v).max() <= np.sqrt(6.0 / fan) * (1 + 1e-6) and np.abs(v).max() > 0.9 * np.sqrt(6.0 / fan)
        else:
            assert np.array_equal(v, b[k]), k


def test_bc_tables_of_an_image_only_agent():
    from serl_amd.agents.flax_tree import bc_paths, bc_shapes
    from serl_amd.utils.init_ref import bc_leaves
    keys = ("wrist", "front")
    sh, full = bc_shapes(keys, 64, 64, 5, 3, use_proprio=False), bc_shapes(keys, 64, 64, 5, 3)
    assert sh["actor/w1"] == (512, 256) and full["actor/w1"] == (576, 256)
    assert set(full) - set(sh) == {"enc/proprio/dense/kernel", "enc/proprio/dense/bias", "enc/proprio/ln/scale", "enc/proprio/ln/bias"}
    paths = bc_paths(keys, use_proprio=False)
    assert set(paths) == set(sh) and not any(p[:3] in (("modules_actor", "encoder", "Dense_0"), ("modules_actor", "encoder", "LayerNorm_0")) for p in paths.values())
    assert [lf.name for lf in bc_leaves(keys, 64, 64, 5, 3, use_proprio=False)] == [k for k in sh if not k.startswith("trunk/")]
    assert bc_paths(keys) == bc_paths(keys, True) and bc_shapes(keys, 64, 64, 5, 3, use_proprio=True) == full


def test_checkpoint_refusal_is_decided_from_the_tree(monkeypatch):
    """load_state_dict on a stand-in agent: a tree of the other kind is refused before any leaf is written"""
    from serl_amd.agents.flax_tree import theta_paths, tree_from_leaves
    from serl_amd.utils.checkpoint import load_state_dict
    keys = ("wrist",)

    def tree(flag):
        kw = {} if flag else {"use_proprio": False}
        sh = pinit.theta_shapes(1, 32, 32, 5, 3, ensemble=2, encoder_type="small", **kw)
        return tree_from_leaves(theta_paths(keys, encoder_type="small", **kw), sh, lambda leaf: np.zeros(int(np.prod(sh[leaf])), np.float32))

    class Core:
        def __init__(self, flag):
            self.use_proprio, self.written = flag, []
            from serl_amd._lib_agent import SerlAgentCfg
            self.cfg = SerlAgentCfg(0, 1, 32, 32, 5, 3, 6, 2, 256, 256, 8, 64)
            self.cfg.encoder_type = 1
            self.leaves = {}

        def set(self, *a):
            self.written.append(a)

    class Agent:
        def __init__(self, flag):
            self.core, self.image_keys = Core(flag), keys
    for have, given, pat in ((True, False, "the state holds no proprio branch"), (False, True, "the state holds the proprio branch")):
        agent = Agent(have)
        with pytest.raises(ValueError, match=pat + ".*nothing was loaded"):
            load_state_dict(agent, {"params": tree(given)})
        assert agent.core.written == []
    agent = Agent(False)
    load_state_dict(agent, {"params": tree(False)})
    assert agent.core.written and not any(a[1].startswith("enc/proprio") for a in agent.core.written)


# ---- the general oracle -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("encoder_type", ["resnet-pretrained", "small"])
def test_general_oracle_with_the_proprio_branch_is_policy_fixeds_bit_for_bit(encoder_type):
    kw = dict(image_keys=("wrist",), H=32, W=32, S=5, A=3, ensemble=2, encoder_type=encoder_type)
    states = []
    for cfg, installed, init in ((IO.ImageOnlyConfig(**kw), IO.installed, IO.init_params), (PF.FixedConfig(**kw), PF.installed, PF.init_params)):
        with installed():
            trunk, theta = init(cfg, 42)
            st = O.TrainState(cfg, trunk, theta, torch.float64)
            b, noise = AH.synth_batch(cfg, 6, seed=4), O.make_noise(cfg, 6, seed=8, utd_ratio=2)
            info, _ = O.update_high_utd(st, AH.batch_to_torch(b, torch.float64), O.noise_to_torch(noise, torch.float64), 2)
            states.append((st, info))
    (a, ia), (b, ib) = states
    assert ia == ib and list(a.params) == list(b.params)
    for k in a.params:
        assert torch.equal(a.params[k], b.params[k]) and torch.equal(a.target[k], b.target[k]), k
    assert O.encode is IO._ORIG["encode"] and O.init_params is IO._ORIG["init_params"]      # the originals are back


def test_the_image_only_oracle_never_reads_the_state():
    with IO.installed():
        cfg, B = IO.case_config("c3_small_1cam_B6_A3_adamw_clip")
        infos = []
        for fill in (None, float("nan")):
            trunk, theta = IO.init_params(cfg, 42)
            st = O.TrainState(cfg, trunk, theta, torch.float64)
            b = AH.synth_batch(cfg, B, seed=4)
            if fill is not None:
                b["state"][:], b["next_state"][:] = fill, fill
            infos.append(O.update_high_utd(st, AH.batch_to_torch(b, torch.float64), O.noise_to_torch(O.make_noise(cfg, B, seed=8, utd_ratio=2), torch.float64), 2)[0])
        assert infos[0] == infos[1] and all(np.isfinite(v) for v in infos[0].values())
        assert O.trainable_param_shapes(cfg)["critic/w1"] == (2, 259, 256)


def test_the_frame_stack_case_keeps_adams_first_step_well_conditioned():
    with IO.installed():
        m = IO.stack_first_step_margin()
    assert m >= IO.ADAM_MARGIN, m


# ---- the reference's own code: tests/golden/imgonly_*.npz --------------------------------------------------------------------------
def _golden_trees():
    """(name, ImageOnlyConfig, the reference's own parameter tree as shapes) of the three DrQ fixtures"""
    import json
    out = [(f"update_{n}", g["cfg"], g["meta"]["param_tree"]) for n in IO.UPDATE_GOLDEN for g in [IO.load_golden(n)]]
    z, cfg, _, _ = IO.init_golden()
    return out + [("init_drq", cfg, json.loads(str(z["meta"]))["param_tree"])]


def test_leaf_tables_match_the_trees_the_reference_built():
    from oracle import golden_update as G
    from serl_amd.agents import flax_tree as FT
    for name, cfg, want in _golden_trees():
        assert cfg.use_proprio is False
        for mod in ("modules_actor", "modules_critic"):
            enc = want[mod].get("encoder", {})
            assert "Dense_0" not in enc and "LayerNorm_0" not in enc, (name, mod)
        kw = NetSpec(use_proprio=False).leaf_kwargs()
        shapes = pinit.theta_shapes(cfg.n_cam, cfg.H, cfg.W, cfg.S, cfg.A, ensemble=cfg.ensemble, encoder_type=cfg.encoder_type, **kw)
        paths = FT.theta_paths(cfg.image_keys, encoder_type=cfg.encoder_type, **kw)
        if cfg.encoder_type != "small":
            shapes.update(pinit.trunk_shapes())
            paths.update({leaf: [("modules_actor", "encoder", f"encoder_{FT.trunk_owner(cfg.image_keys)}", "pretrained_encoder") + sub]
                          for leaf, sub in FT._trunk_paths().items()})
        got = G.shape_tree(FT.tree_from_leaves(paths, shapes, lambda leaf: np.zeros(int(np.prod(shapes[leaf])), np.float32)))
        assert got == want, name
        assert tuple(want["modules_actor"]["network"]["Dense_0"]["kernel"]) == (256 * cfg.n_cam, 256)
        assert tuple(want["modules_critic"]["network"]["Dense_0"]["kernel"]) == (cfg.ensemble, 256 * cfg.n_cam + cfg.A, 256)


def test_host_twins_equal_the_reference_initial_params_of_the_image_only_tree():
    import init_golden_helpers as IG
    from serl_amd.utils import init_ref as IR
    z, cfg, recs, shapes = IO.init_golden()
    assert not any(k.startswith("enc/proprio") for k in recs) and shapes["critic/w1"] == (cfg.ensemble, 256 + cfg.A, 256)
    got = IR.theta_reference(cfg.image_keys, cfg.H, cfg.W, cfg.S, cfg.A, 0, ensemble=cfg.ensemble, encoder_type=cfg.encoder_type,
                             temperature_init=1e-2, device=None, use_proprio=False)
    assert set(got) == set(recs), sorted(set(got) ^ set(recs))
    bad = [m for m in (IG.mismatch(n, recs[n], got[n]) for n in sorted(recs)) if m]
    assert not bad, bad
    for n, v in got.items():
        assert tuple(v.shape) == shapes[n], (n, v.shape, shapes[n])
    assert np.array_equal(IR.create_rng_of(0), z["init_rng"])


@pytest.mark.parametrize("name", IO.UPDATE_GOLDEN)
def test_general_oracle_reproduces_the_reference_golden(name):
    from oracle import golden_update as G
    from test_reference_update import F64_TOL, _oracle_sections, _run_oracle
    g = IO.load_golden(name)
    cfg = g["cfg"]
    with IO.installed():
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
    print(f"imgonly_update_{name}: general oracle vs reference golden, worst {worst:.1e}")
