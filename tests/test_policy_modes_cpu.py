"""CPU: the policy distributions beside the launcher's (tests/policy_modes.py) -- what the committed policy_*.npz fixtures record
about the reference's runs, the flax mapping of the "uniform" tree against the tree the reference built, and the host-side
initialisation of a "uniform" agent."""
import numpy as np
import pytest

from oracle import drq_oracle as O
import golden_replay as GR
import policy_modes as PM

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
    _, meta, z = GR.load_variant("policy", name)
    pol = meta["policy"]
    assert (pol["std_parameterization"], pol["tanh_squash_distribution"], pol["regime"]) == (std, squash, regime)
    assert int(z["policy_n_sample"]) == n_sample and pol["clip_cycle"] == list(PM.CLIP_CYCLE) and pol["log_stds_seed"] == PM.LOG_STDS_SEED
    assert meta["B"] == B and [s[0] for s in meta["schedule"]] == [s[0] for s in sched]
    actor = meta["param_tree"]["modules_actor"]
    if std == "uniform":
        assert pol["std_leaves"] == "log_stds" and actor["log_stds"] == [cfg.A] and "Dense_1" not in actor
    else:
        assert pol["std_leaves"] == "Dense_1" and actor["Dense_1"]["kernel"] == [cfg.hidden, cfg.A] and "log_stds" not in actor
    # the final state holds exactly the leaves of that tree
    stored = {k[2:].split("|")[1] for k in z.files if k.startswith("f_params|")}
    assert stored == set(PM.leaf_names(cfg, std))
    if regime == "trained":
        low, high = z["policy_clip_low"], z["policy_clip_high"]
        assert low.shape == high.shape == (pol["policy_evaluations"], cfg.A) and len(low) >= len(sched)
        for lo, hi in zip(low, high):      # the fixture's condition, in every policy evaluation of every step
            assert (lo == 1.0).sum() >= 1 and (hi == 1.0).sum() >= 1 and ((lo == 0.0) & (hi == 0.0)).sum() >= 2, (lo, hi)
    else:
        assert "policy_clip_low" not in z.files


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
    assert set(th) == set(PM.leaf_names(cfg, "uniform")) and list(O.trainable_param_shapes(cfg))[-1] == PM.leaf_names(cfg, "uniform")[-1]
