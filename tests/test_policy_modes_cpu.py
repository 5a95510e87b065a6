"""CPU: the policy distributions beside the launcher's (tests/policy_modes.py) -- what the committed policy_*.npz fixtures record
about the reference's runs, the oracle's update code in every mode against them, the flax mapping of the "uniform" tree against
the tree the reference built, and the host-side initialisation of a "uniform" agent."""
import numpy as np
import pytest
import torch

from oracle import drq_oracle as O
from oracle import golden_update as G
from oracle import ref_update_runner as RR
import golden_replay as GR
import policy_modes as PM
from test_reference_update import F64_TOL, _oracle_sections

from serl_amd.agents import flax_tree as FT
from serl_amd.utils import init as pinit
from serl_amd.utils import init_ref as IR


def _leaf_paths(tree, prefix=()):
    for k, v in tree.items():
        if isinstance(v, dict):
            yield from _leaf_paths(v, prefix + (k,))
        else:
            yield prefix + (k,), tuple(v)


@pytest.mark.parametrize("name", list(PM.GOLDEN))
def test_golden_records_the_mode_the_reference_ran(name):
    cfg, B, sched, (std, squash), regime, n_sample = PM.GOLDEN[name]
    g, meta, z = GR.load_variant("policy", name)
    pol = meta["policy"]
    assert (pol["std_parameterization"], pol["tanh_squash_distribution"], pol["regime"]) == (std, squash, regime)
    assert (cfg.std_parameterization, cfg.tanh_squash) == (std, squash) and g["cfg"] == cfg
    assert int(z["policy_n_sample"]) == n_sample and pol["clip_cycle"] == list(PM.CLIP_CYCLE) and pol["log_stds_seed"] == PM.LOG_STDS_SEED
    assert meta["B"] == B and [s[0] for s in meta["schedule"]] == [s[0] for s in sched]
    actor = meta["param_tree"]["modules_actor"]
    if std == "uniform":
        assert pol["std_leaves"] == "log_stds" and actor["log_stds"] == [cfg.A] and "Dense_1" not in actor
    else:
        assert pol["std_leaves"] == "Dense_1" and actor["Dense_1"]["kernel"] == [cfg.hidden, cfg.A] and "log_stds" not in actor
    # the final state holds exactly the leaves of that tree
    stored = {k[2:].split("|")[1] for k in z.files if k.startswith("f_params|")}
    assert stored == set(O.trainable_param_shapes(cfg))
    if regime == "trained":
        low, high = z["policy_clip_low"], z["policy_clip_high"]
        assert low.shape == high.shape == (pol["policy_evaluations"], cfg.A) and len(low) >= len(sched)
        for lo, hi in zip(low, high):      # the fixture's condition, in every policy evaluation of every step
            assert (lo == 1.0).sum() >= 1 and (hi == 1.0).sum() >= 1 and ((lo == 0.0) & (hi == 0.0)).sum() >= 2, (lo, hi)
    else:
        assert "policy_clip_low" not in z.files


@pytest.mark.parametrize("name", list(PM.GOLDEN))
def test_oracle_reproduces_the_reference_golden_in_mode(name):
    """tests/test_reference_update.py::test_oracle_reproduces_the_reference_golden on policy_<name>.npz: the oracle's own update
    code, with the distribution read from the Config, against the reference's run in that mode -- every info scalar and the whole
    final state within F64_TOL.  Measured over the seven fixtures: infos 2.4e-13, final state 1.7e-12."""
    g, meta, _ = GR.load_variant("policy", name)
    st = O.TrainState(g["cfg"], *PM.initial_leaves(name), torch.float64)
    worst_i = 0.0

    def check(i, step, info):
        nonlocal worst_i
        assert set(info) == {k for k in step["info"] if not k.endswith("_lr")}
        for k, v in info.items():
            r = step["info"][k]
            worst_i = max(worst_i, abs(v - r) / max(1.0, abs(r)))
            assert abs(v - r) <= F64_TOL * max(1.0, abs(r)), (i, k, v, r)
    RR.run_steps(st, g["steps"], torch.float64, on_info=check)
    assert st.step == meta["final_step"]
    worst = 0.0
    for sec, tree in _oracle_sections(st).items():
        assert set(g["final"][sec]) == set(tree), sec
        for leaf, t in tree.items():
            e, how = G.leaf_compare(f"{sec}/{leaf}", g["final"][sec][leaf], t.numpy())
            assert e < F64_TOL, (sec, leaf, how, e)
            worst = max(worst, e)
    print(f"policy_{name}: oracle vs reference golden, infos {worst_i:.1e}, final state {worst:.1e}")


def test_uniform_replaces_the_log_std_dense_in_its_arena_position():
    """O.trainable_param_shapes is the one statement of the "uniform" tree: actor/log_stds [A] where the Dense's two leaves stood,
    every other leaf in place; O.init_params draws the shared leaves as for "exp" and leaves log_stds at the reference's zeros"""
    for base in (O.Config(image_keys=(), S=10, A=5), O.Config(image_keys=("image",), H=64, W=64, S=5, A=3)):
        uni = PM.mode_config("uniform", True, **{k: getattr(base, k) for k in ("image_keys", "H", "W", "S", "A")})
        exp, got = list(O.trainable_param_shapes(base)), O.trainable_param_shapes(uni)
        i = exp.index(PM.STD_DENSE[0])
        assert exp[i:i + 2] == list(PM.STD_DENSE) and list(got) == exp[:i] + ["actor/log_stds"] + exp[i + 2:]
        assert got["actor/log_stds"] == (base.A,)
        (tr_e, th_e), (tr_u, th_u) = O.init_params(base, 3), O.init_params(uni, 3)
        assert list(th_u) == list(got) and not th_u["actor/log_stds"].any() and th_u["actor/log_stds"].dtype == np.float32
        assert all(np.array_equal(th_u[k], th_e[k]) for k in th_u if k != "actor/log_stds")
        assert all(np.array_equal(tr_u[k], tr_e[k]) for k in tr_e)


@pytest.mark.parametrize("name", [n for n in PM.GOLDEN if PM.GOLDEN[n][3][0] == "uniform"])
def test_flax_paths_of_a_uniform_agent_equal_the_recorded_tree(name):
    cfg = PM.GOLDEN[name][0]
    tree = GR.load_variant("policy", name)[1]["param_tree"]
    etype = cfg.encoder_type
    paths = FT.theta_paths(cfg.image_keys, encoder_type=etype, std_parameterization="uniform")
    shapes = pinit.theta_shapes(cfg.n_cam, cfg.H, cfg.W, cfg.S, cfg.A, ensemble=cfg.ensemble, hidden=cfg.hidden, encoder_type=etype,
                                std_parameterization="uniform")
    assert set(paths) == set(shapes) and "actor/log_stds" in paths and not any("logstd" in k for k in paths)
    assert paths["actor/log_stds"] == [("modules_actor", "log_stds")]
    want = {p: s for p, s in _leaf_paths(tree) if "pretrained_encoder" not in p}
    got = {ps[0]: tuple(shapes[leaf]) for leaf, ps in paths.items()}
    assert got == want
    # ... and the default arguments still give the tree every other caller sees
    assert "actor/logstd/kernel" in FT.theta_paths(cfg.image_keys, encoder_type=etype)
    assert "actor/logstd/kernel" in pinit.theta_shapes(cfg.n_cam, cfg.H, cfg.W, cfg.S, cfg.A, encoder_type=etype)


@pytest.mark.parametrize("keys", [(), ("image",)], ids=["state", "one_cam"])
def test_host_init_of_a_uniform_agent_shares_every_other_leaf_with_the_exp_agent(keys, monkeypatch):
    """param_init="reference" (threefry): flax keys depend on a module's own path and counter, so dropping Dense_1 moves no other
    leaf; log_stds is zeros (actor_critic_nets.py:199-201).  The numpy initialisation has the same property."""
    H = W = 64 if keys else 0
    S, A = 5, 3
    exp = IR.theta_reference(keys, H, W, S, A, 0, ensemble=4, device=None)
    for std in ("softplus", "uniform"):
        got = IR.theta_reference(keys, H, W, S, A, 0, ensemble=4, device=None, std_parameterization=std)
        shared = [k for k in exp if k in got]
        if std == "uniform":
            assert set(exp) - set(got) == set(PM.STD_DENSE) and set(got) - set(exp) == {"actor/log_stds"}
            assert got["actor/log_stds"].shape == (A,) and got["actor/log_stds"].dtype == np.float32 and not got["actor/log_stds"].any()
        else:
            assert set(exp) == set(got)
        for k in shared:
            assert np.array_equal(exp[k].view(np.uint32), got[k].view(np.uint32)), (std, k)
    a = pinit.init_theta(len(keys), H, W, S, A, seed=3, ensemble=4)
    b = pinit.init_theta(len(keys), H, W, S, A, seed=3, ensemble=4, std_parameterization="uniform")
    assert not b["actor/log_stds"].any() and set(a) - set(b) == set(PM.STD_DENSE)
    for k in b:
        if k != "actor/log_stds":
            assert np.array_equal(a[k], b[k]), k


def test_policy_kwargs_are_read_as_the_launcher_writes_them():
    assert pinit.policy_mode(None) == pinit.policy_mode({}) == ("exp", True)
    assert pinit.policy_mode(PM.policy_kwargs("uniform", False)) == ("uniform", False)
    with pytest.raises(NotImplementedError, match="fixed"):
        pinit.policy_mode({"std_parameterization": "fixed", "fixed_std": 0.1})
    with pytest.raises(NotImplementedError, match="fixed_std"):
        pinit.policy_mode({"fixed_std": 0.1})


def test_mode_theta_is_what_the_fixtures_started_from():
    cfg = PM.GOLDEN["trained_sac_state_uniform"][0]
    _, th = PM.initial_leaves("trained_sac_state_uniform")
    assert list(th["actor/log_stds"]) == [PM.CLIP_CYCLE[j % 4] for j in range(cfg.A)] and not any(k in th for k in PM.STD_DENSE)
    _, th = PM.initial_leaves("trained_sac_state_softplus")
    assert list(th["actor/logstd/bias"]) == [PM.CLIP_CYCLE[j % 4] for j in range(cfg.A)]
    _, th = PM.initial_leaves("update_sac_state_uniform")
    assert th["actor/log_stds"].min() >= -1.5 and th["actor/log_stds"].max() < 0.5 and len(set(th["actor/log_stds"])) == cfg.A
    assert set(th) == set(O.trainable_param_shapes(cfg)) and list(O.trainable_param_shapes(cfg))[-1] == "temp/lagrange"
