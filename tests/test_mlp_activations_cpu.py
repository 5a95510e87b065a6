"""CPU: the activations of the critic's and the policy's MLP beside the launcher's tanh -- relu and swish (= silu), chosen per network
(networks/mlp.py:19-31; tests/mlp_activations.py).

* tests/golden/act_*.npz were produced by tests/golden/make_golden_update_activations.py from the reference's own update code with
  `activations` overridden in the kwargs its factories pass; the oracle (oracle.drq_oracle's policy_head / critic_forward with
  the Config's activations, autograd for the backward) reproduces them within F64_TOL of tests/test_reference_update.py, the bound
  of every oracle-against-golden test here.  That pins the statement the GPU tests compare with at other widths.
* utils.init.mlp_activations reads the two kwargs as the reference's MLP would and refuses the rest from the arguments alone.
* serl_agent_create_mlp is declared, exported and bound; the entries it generalises are still there.

The two fixtures with a relu network, act_update_sac_state_relu and act_update_sac_state_mixed, carry the condition that the smallest
|pre-activation| of every evaluation of the reference's run is at least 1e-4.  From O.init_params' LayerNorm leaves no batch seed
meets it (8e6 relu pre-activations per run of density 0.4 at 0: over the seeds 100, 116, ..., 244 the smallest lay between 5.4e-9
and 1.0e-6), so their runs start from mlp_activations.kink_margin's leaves: four live columns per LayerNorm vector, off in 40 % of
the rows, every other column on in all rows or off in all rows.  The generator's seed search then ended at batch seed 1780 (106
seeds tried) and 1460 (86 tried); smallest |pre-activation| 1.0022e-4 and 1.0005e-4."""
import dataclasses
import json
import os
import re

import numpy as np
import pytest
import torch

from oracle import drq_oracle as O
from oracle import golden_update as G
from oracle import ref_update_runner as RR
import golden_replay as GR
import mlp_activations as MA
import mlp_widths as MW
from serl_amd.utils import init as pinit
from test_mlp_widths_cpu import REFUSALS, _create_drq, _create_states
from test_reference_update import F64_TOL, _oracle_sections

SERVED = 'served: activations "tanh", "relu", "swish" (= "silu") by name or as a callable of that __name__, dropout_rate None or 0'


def _need_golden(name):
    assert os.path.exists(GR.variant_path("act", name)), f"act_{name}.npz is not recorded"


# ---- the restatement against the reference's own runs ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MA.GOLDEN))
def test_restated_mlps_reproduce_the_reference_golden(name):
    _need_golden(name)
    cfg, B, sched, (critic, policy), regime, n_sample = MA.GOLDEN[name]
    g, meta, z = GR.load_variant("act", name)
    act = meta["activations"]
    assert (act["critic"], act["policy"], act["regime"]) == (critic, policy, regime) and int(z["act_n_sample"]) == n_sample
    assert g["cfg"] == cfg and g["B"] == B and [s["kind"] for s in g["steps"]] == [s[0] for s in sched] and g["meta"]["batch_seed"] == act["batch_seed"]
    if "relu" in (critic, policy):      # the fixture's condition, as the generator recorded it; and the kink was crossed
        assert act["relu_min_abs_pre"] >= MA.KINK_MIN and regime == "kink_margin" and act["margin_seed"] == MA.MARGIN_SEED, act
        assert all(0.2 < f < 0.6 for f in act["relu_off_fraction"].values()) and set(act["relu_off_fraction"]) == \
            {w for w, a in (("critic", critic), ("policy", policy)) if a == "relu"}, act
    if regime == "trained":             # swish's saturated branch is exercised
        assert max(act["max_abs_pre"].values()) >= 10.0, act
    trunk, theta = MA.initial_leaves(name)
    st = O.TrainState(g["cfg"], trunk, theta, torch.float64)
    recs = {"critic": MA.Recorder(), "policy": MA.Recorder()}
    def check(i, step, info):
        for k, v in info.items():
            r = step["info"][k]
            assert abs(v - r) <= F64_TOL * max(1.0, abs(r)), (i, k, v, r)
    with O.observe_preactivations(recs):
        RR.run_steps(st, g["steps"], torch.float64, on_info=check)
    assert not O.OBSERVERS      # nothing observes once the block is left
    assert st.step == g["meta"]["final_step"]
    # the restatement saw the pre-activations the reference's activation saw
    for w, rec in recs.items():
        assert abs(max(rec.max_abs) - act["max_abs_pre"][w]) <= 1e-9 * max(rec.max_abs), (w, max(rec.max_abs), act["max_abs_pre"][w])
        assert abs(min(rec.min_abs) - act["min_abs_pre"][w]) <= 1e-9, (w, min(rec.min_abs), act["min_abs_pre"][w])
        if w in act.get("relu_off_fraction", {}):
            assert abs(rec.off_fraction - act["relu_off_fraction"][w]) < 1e-12, (w, rec.off_fraction)
    worst = 0.0
    for sec, tree in _oracle_sections(st).items():
        assert set(g["final"][sec]) == set(tree), sec
        for leaf, t in tree.items():
            e, how = G.leaf_compare(f"{sec}/{leaf}", g["final"][sec][leaf], t.numpy())
            assert e < F64_TOL, (sec, leaf, how, e)
            worst = max(worst, e)
    print(f"act_{name}: restated MLPs vs reference golden, worst {worst:.1e}")


@pytest.mark.parametrize("name", [n for n in MA.GOLDEN if os.path.exists(GR.variant_path("act", n))])
def test_golden_differs_from_the_tanh_run(name):
    """the activation took effect in the reference: the oracle with the launcher's tanh MLPs does NOT reproduce the first step's
    critic loss (a missing fixture fails in the test above)"""
    g = GR.load_variant("act", name)[0]
    trunk, theta = MA.initial_leaves(name)
    cfg = dataclasses.replace(g["cfg"], critic_activation="tanh", policy_activation="tanh")
    st = O.TrainState(cfg, trunk, theta, torch.float64)
    (info,) = RR.run_steps(st, g["steps"][:1], torch.float64)
    r = g["steps"][0]["info"]["critic_loss"]
    assert abs(info["critic_loss"] - r) > 1e-3 * abs(r), (info["critic_loss"], r)


def test_restatement_with_tanh_is_the_oracle():
    """The default Config is the launcher's tanh and observing changes no value: the two MLPs under Recorders, bit for bit.  (The
    oracle's update code against what the per-option restatements it replaced computed was compared once, over every policy_*,
    act_* and wd_* fixture, when they were folded into it: every info scalar, leaf and moment np.array_equal.)"""
    cfg = O.Config(image_keys=(), S=10, A=5)
    assert (cfg.critic_activation, cfg.policy_activation, cfg.std_parameterization, cfg.tanh_squash) == ("tanh", "tanh", "exp", True)
    th = O.to_torch(O.init_params(cfg, 3)[1], torch.float64)
    enc, a = torch.randn(7, cfg.S, dtype=torch.float64), torch.randn(7, cfg.A, dtype=torch.float64)
    want = O.policy_head(th, cfg, enc), O.critic_forward(th, cfg, enc, a)
    recs = {"critic": MA.Recorder(), "policy": MA.Recorder()}
    with O.observe_preactivations(recs):
        got = O.policy_head(th, cfg, enc), O.critic_forward(th, cfg, enc, a)
    assert torch.equal(got[0][0], want[0][0]) and torch.equal(got[0][1], want[0][1]) and torch.equal(got[1], want[1])
    assert len(recs["critic"].min_abs) == len(recs["policy"].min_abs) == 2 and not O.OBSERVERS
    with pytest.raises(MA.Kink):      # an observer's exception leaves the hook empty too
        with O.observe_preactivations({"policy": MA.Recorder(floor=1e9)}):
            O.policy_head(th, cfg, enc)
    assert not O.OBSERVERS
    # relu's gradient at exactly 0 is 0 (jax.nn.relu's choice), and swish is x * sigmoid(x)
    x = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    O.ACTIVATIONS["relu"](x).sum().backward()
    assert not x.grad.any()
    v = torch.tensor([-30.0, -1.0, 0.0, 2.0], dtype=torch.float64)
    assert torch.allclose(O.ACTIVATIONS["swish"](v), torch.nn.functional.silu(v), rtol=1e-15, atol=0)


# ---- reading the kwargs ----------------------------------------------------------------------------------------------------------
def _named(name):
    def fn(x):
        return x
    fn.__name__ = name
    return fn


def test_mlp_activations_reads_strings_callables_and_absent_keys():
    assert pinit.MLP_ACTIVATIONS == ("tanh", "relu", "swish")       # SERL_ACT_TANH / _RELU / _SWISH = 0 / 1 / 2
    assert pinit.mlp_activations(None, None) == pinit.mlp_activations({}, {}) == ("tanh", "tanh")
    assert pinit.mlp_activations(MW.mlp_kwargs(256), MW.mlp_kwargs(256)) == ("tanh", "tanh")        # what the launcher writes
    for name, want in (("tanh", "tanh"), ("relu", "relu"), ("swish", "swish"), ("silu", "swish")):
        assert pinit.mlp_activations({"activations": name}, None) == (want, "tanh")
        assert pinit.mlp_activations(None, {"activations": _named(name)}) == ("tanh", want)
    assert pinit.mlp_activations({"activations": torch.relu}, {"activations": torch.nn.functional.silu}) == ("relu", "swish")
    assert pinit.mlp_activations({"activations": torch.tanh, "dropout_rate": None}, {"activations": "swish", "dropout_rate": 0.0}) == \
        ("tanh", "swish")
    assert pinit.mlp_activations(MA.network_kwargs("relu"), MA.network_kwargs("swish")) == ("relu", "swish")


BAD = [("gelu", {"activations": "gelu"}, "activations='gelu'"),
       ("lambda", {"activations": lambda x: x}, "activations=<function"),
       ("dropout", {"activations": "swish", "dropout_rate": 0.1}, "dropout_rate=0.1"),
       ("not_callable", {"activations": 3}, "activations=3"),
       ("dropout_not_a_number", {"dropout_rate": "0.1"}, "dropout_rate='0.1'")]


@pytest.mark.parametrize("which", ["critic_network_kwargs", "policy_network_kwargs"])
@pytest.mark.parametrize("kw,message", [b[1:] for b in BAD], ids=[b[0] for b in BAD])
def test_mlp_activations_refuses_what_is_not_served(which, kw, message):
    args = {"critic_network_kwargs": {}, "policy_network_kwargs": {}, which: kw}
    with pytest.raises(NotImplementedError, match=re.escape(f"{which}: {message}")) as e:
        pinit.mlp_activations(**args)
    assert SERVED in str(e.value)


@pytest.mark.parametrize("create", [_create_states, _create_drq], ids=["create_states", "create_drq"])
@pytest.mark.parametrize("kw,message", [b[1:] for b in BAD[:3]], ids=[b[0] for b in BAD[:3]])
def test_create_refuses_from_the_arguments_alone(create, kw, message):
    """no device is touched (this test runs without one)"""
    with pytest.raises(NotImplementedError, match=re.escape(message)) as e:
        create(policy_kwargs=dict(MW.POLICY_KWARGS), critic_network_kwargs={**MW.mlp_kwargs(128), **kw},
               policy_network_kwargs=MW.mlp_kwargs(128))
    assert SERVED in str(e.value)


@pytest.mark.parametrize("create", [_create_states, _create_drq], ids=["create_states", "create_drq"])
@pytest.mark.parametrize("act", ["relu", "swish"])
@pytest.mark.parametrize("kw,message", [r[1:] for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_width_refusals_keep_their_messages_beside_a_served_activation(create, act, kw, message):
    kw = {k: ({**v, "activations": act} if k.endswith("network_kwargs") else v) for k, v in kw.items()}
    with pytest.raises(NotImplementedError, match=message) as e:
        create(policy_kwargs=dict(MW.POLICY_KWARGS), **kw)
    assert "served: hidden_dims=[h, h] with LayerNorm, h a multiple of 64 in [64, 1024], the same h for critic and policy" in str(e.value)


def test_earlier_refusals_still_come_first():
    """a bad activation does not overtake the checks that were there: encoder type, use_proprio, the policy distribution, the width"""
    from serl_amd.agents.drq import DrQAgent
    from serl_amd.agents.sac import SACAgent
    obs = {"image": np.zeros((1, 64, 64, 3), np.uint8), "state": np.zeros((1, 5), np.float32)}
    bad = {"activations": "gelu"}
    with pytest.raises(NotImplementedError, match="Unknown encoder type: bogus"):
        DrQAgent.create_drq(0, obs, np.zeros((3,), np.float32), encoder_type="bogus", use_proprio=True, critic_network_kwargs=bad)
    with pytest.raises(NotImplementedError, match="only use_proprio=True"):
        DrQAgent.create_drq(0, obs, np.zeros((3,), np.float32), encoder_type="small", use_proprio=False, critic_network_kwargs=bad)
    for create in (lambda **k: DrQAgent.create_drq(0, obs, np.zeros((3,), np.float32), encoder_type="small", use_proprio=True, **k),
                   lambda **k: SACAgent.create_states(0, np.zeros((10,), np.float32), np.zeros((4,), np.float32), **k)):
        with pytest.raises(NotImplementedError, match="std_parameterization='fixed'"):
            create(policy_kwargs={"std_parameterization": "fixed"}, critic_network_kwargs=bad)
        with pytest.raises(NotImplementedError, match="has 3 layers"):
            create(critic_network_kwargs={**bad, "hidden_dims": [64, 64, 64]})


# ---- the C ABI, as far as no device is needed ------------------------------------------------------------------------------------
def test_create_mlp_is_declared_exported_and_bound():
    from serl_amd import _lib, _lib_agent
    L = _lib.lib()
    decl = _lib.exported_symbols()
    for name in ("serl_agent_create", "serl_agent_create_policy", "serl_agent_create_mlp"):
        assert hasattr(L, name) and name in decl and name in _lib_agent.SIGNATURES, name
    assert decl["serl_agent_create"] == len(_lib_agent.SIGNATURES["serl_agent_create"]) == 2
    assert decl["serl_agent_create_policy"] == len(_lib_agent.SIGNATURES["serl_agent_create_policy"]) == 4
    assert decl["serl_agent_create_mlp"] == len(_lib_agent.SIGNATURES["serl_agent_create_mlp"]) == 6
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "serl_mi355.h")).read()
    for i, name in enumerate(("SERL_ACT_TANH", "SERL_ACT_RELU", "SERL_ACT_SWISH")):
        assert re.search(rf"#define {name} {i}\b", header), name
        assert pinit.MLP_ACTIVATIONS[i] == name[9:].lower()
    assert "int serl_agent_create_mlp(const serl_agent_cfg* cfg, int std_param, int no_tanh, int critic_act, int policy_act, serl_agent** out);" in header
    assert _lib_agent.SerlAgentCfg._fields_[-1][0] == "num_stack"       # the struct is the one it was


def test_golden_files_stay_out_of_the_update_sweeps_and_under_the_size_limit():
    for name in MA.GOLDEN:
        path = GR.variant_path("act", name)
        assert os.path.basename(path).startswith("act_")
        if os.path.exists(path):
            assert os.path.getsize(path) < 1 << 20
            meta = json.loads(str(np.load(path)["meta"]))
            assert meta["activations"]["transform"] == "mlp_activations.act_theta"


def test_kink_margin_leaves_are_what_the_relu_fixtures_started_from():
    cfg = MA.GOLDEN["update_sac_state_relu"][0]
    _, th = MA.initial_leaves("update_sac_state_relu")
    _, base = O.init_params(cfg, GR.PARAM_SEED)
    for k, v in th.items():
        if k.split("/")[-2] in ("ln1", "ln2"):
            rows = v.reshape(-1, v.shape[-1])
            live = (th[k.rsplit("/", 1)[0] + "/scale"].reshape(rows.shape) == 1.0)
            assert (live.sum(1) == MA.GOLDEN_LIVE).all(), k          # live columns per vector (per member in the critic)
            if k.endswith("scale"):
                assert (rows[~live] == np.float32(MA.safe_scale(cfg.hidden))).all() and MA.safe_scale(cfg.hidden) == MA.SAFE_SCALE
            else:
                assert (rows[live] == np.float32(MA.LIVE_BIAS)).all() and (np.abs(rows[~live]) == MA.SAFE_BIAS).all()
                assert 0.3 < (rows[~live] > 0).mean() < 0.7          # units on in every row and units off in every row
        else:
            assert np.array_equal(v, np.asarray(base[k], np.float32)), k
    # a safe column cannot reach 0 at any width: |xhat| <= sqrt(D - 1)
    for D in pinit.HIDDEN_WIDTHS:
        assert MA.SAFE_BIAS - MA.safe_scale(D) * np.sqrt(D - 1) >= 0.2 - 1e-12, D


def test_every_relu_row_case_of_the_gpu_tests_finds_its_seed():
    """the fp64 side of tests/test_mlp_activations_gpu.py's row cases (no GPU needed): with kink_margin's leaves every case with a
    relu network has a batch seed among the ten whose relu pre-activations all stay KINK_MIN away from 0, so none of them skips;
    and the live units are off in some rows and on in others"""
    import test_mlp_activations_gpu as TG
    for label, hidden, B in TG.ROWS:
        for critic, policy in TG.PAIRS:
            k, side = TG._oracle_side(hidden, B, critic, policy, MA.KINK_MIN)
            assert k is not None, (label, critic, policy, side)
            if "relu" in (critic, policy):
                for w, a in (("critic", critic), ("policy", policy)):
                    if a == "relu":
                        assert min(side["recs"][w].min_abs) >= MA.KINK_MIN and 0.05 < side["recs"][w].off_fraction < 0.95, \
                            (label, w, side["recs"][w].off_fraction)
            print(f"{label} critic={critic} policy={policy}: seed index {k}")
