"""GPU: critic and policy MLP widths above 1024 (serl_agent_opts.wide_widths, mlp_wide=True) under the whole update chain, on the
case table of tests/mlp_wide.py: the rows one workgroup of four waves owns (serl_amd/csrc/ln_wide.h).  TOL = 1e-4 as in
tests/test_mlp_shapes_gpu.py; every figure of every case measured below it (WIDE WIDTHS), so it is asserted as it
stands.  Without the switch every test fails when its agent is made (AgentCore has no `wide`)."""
import numpy as np
import pytest
import torch

from oracle import drq_oracle as O
import agent_helpers as AH
import mlp_ragged as MR
import mlp_shapes as MS
import mlp_wide as MW
import policy_fixed as PF
from test_agent_gpu import _compare_state
from test_chain_fusion_gpu import _assert_state_bits, _bits_equal, _launches
from test_mlp_widths_gpu import _Figures, _flat_batch, _info

pytestmark = pytest.mark.gpu
_SAC = dict(S=10, A=4, B=8, critic_ensemble_size=2, mlp_ragged=True, mlp_wide=True)


@pytest.fixture(autouse=True)
def _general_oracle():
    with MW.installed():
        yield


@pytest.mark.parametrize("name", list(MW.CASES))
def test_updates_match_the_oracle_in_both_schedules(gpu, name):
    """update_critics, update_high_utd(1) and the case's UTD: fused == un-fused bit for bit; info scalars, q, target_q, every
    gradient leaf (through the storage layout, pads asserted zero) and the state after the step against the fp64 oracle"""
    for call in MW.case_config(name)[2]:
        run = MW.oracle_run(name, call)
        cfg, B, aux, crit = run["cfg"], run["B"], run["aux"], call == "critics"
        cores = [MW.make_core(cfg, B, run["seed"], fuse=f) for f in (True, False)]
        for core in cores:
            db, dn = AH.batch_to_device(cfg, run["batch"]), AH.noise_to_device(cfg, run["noise"])
            core.update_critics(db, dn) if crit else core.update_high_utd(db, call[1], dn)
        core, tap = cores[0], "g_critic" if crit else "g_actor"
        lo, hi = MR.tap_ranges(core)[tap]
        assert _bits_equal(core.debug(tap, hi - lo), cores[1].debug(tap, hi - lo)) and core.read_info() == cores[1].read_info(), (name, call)
        _assert_state_bits(cfg, core, cores[1], (name, call))
        fig = _Figures(f"{name} {call}")
        _info(fig, core.read_info(), run["info"], ("critic_loss", "predicted_qs", "target_qs") + (() if crit else (
            "actor_loss", "temperature", "entropy", "temperature_loss")))
        if crit:
            fig.add("q", AH.rel_err(core.debug("q", cfg.ensemble * B).reshape(cfg.ensemble, B), aux["q"].numpy()))
            fig.add("target_q", AH.rel_err(core.debug("target_q", B), aux["target_q"].numpy()))
        MR.grads(fig, cfg, core, aux["grads" if crit else "g_actor"], tap)
        fig.check()
        _compare_state(cfg, run["state"], core, steps=1 if crit else call[1] + 1)
        assert core.step == run["state"].step and core.debug("ctr_nonzero", 1)[0] == 0 and core.pad_max_abs == 0.0


def _two_updates(cfg, B, core):
    torch.cuda.synchronize()
    l0 = _launches()
    for it in range(2):
        core.update_high_utd(AH.batch_to_device(cfg, AH.synth_batch(cfg, B, seed=300 + it)), 2,
                             AH.noise_to_device(cfg, O.make_noise(cfg, B, seed=400 + it, utd_ratio=2)))
    torch.cuda.synchronize()
    return _launches() - l0


def test_1024_with_the_switch_is_the_agent_without_it_and_2048_launches_no_more(gpu):
    cfg, cfg2 = (PF.FixedConfig(**MS.config("state", (h, h), (h, h), ensemble=2).__dict__) for h in (1024, 2048))
    on, off = (MW.make_core(cfg, 6, 42, wide=w) for w in (True, False))
    assert on.spec.to_c().wide_widths == 1 and off.spec.to_c().wide_widths == 0
    n = _two_updates(cfg, 6, on), _two_updates(cfg, 6, off), _two_updates(cfg2, 6, MW.make_core(cfg2, 6, 42))
    assert on.read_info() == off.read_info() and n[0] == n[1] == n[2], n
    _assert_state_bits(cfg, on, off, "1024")


def test_get_set_and_checkpoint_roundtrip_of_a_wide_agent(gpu, tmp_path):
    from serl_amd.agents.flax_tree import net_spec_of
    from serl_amd.utils.checkpoint import restore_checkpoint, save_checkpoint
    agent, again = (MS.sac_agent((1088, 2048), (1100,), seed=s, **_SAC) for s in (7, 2))
    core = agent.core
    assert core.critic_dims == (1088, 2048) and core.policy_dims == (1100,) and core.spec.wide and core.spec.ragged and net_spec_of(core).wide
    assert agent.state.params["modules_critic"]["network"]["Dense_1"]["kernel"].shape == (2, 1088, 2048)
    for leaf in ("critic/w2", "critic/ln2/scale", "actor/w1", "actor/mean/kernel"):
        x = (np.random.default_rng(5).standard_normal(core.leaves[leaf]) * 0.05 + 1.0).astype(np.float32)
        core.set("params", leaf, x)
        assert _bits_equal(core.get("params", leaf), x) and core.pad_max_abs == 0.0, leaf
    agent.update_high_utd(_flat_batch(10, 4, 8, 10), utd_ratio=2)
    save_checkpoint(str(tmp_path / "wide"), agent, step=agent.state.step)
    restore_checkpoint(str(tmp_path / "wide"), again, restore_rng=True)
    for a in (agent, again):
        a.update_high_utd(_flat_batch(10, 4, 8, 20), utd_ratio=1)
    want = MR.all_bits(core)
    assert all(_bits_equal(v, want[key]) for key, v in MR.all_bits(again.core).items()) and again.core.pad_max_abs == 0.0


def test_candidate_actions_are_refused_at_a_wide_first_critic_layer_alone(gpu):
    from serl_amd import _lib
    state, acts, eps = torch.zeros((2, 10), device="cuda"), torch.zeros((2, 4, 4), device="cuda"), torch.zeros((4, 2, 4), device="cuda")
    wide, served = (MW.make_core(PF.FixedConfig(**MS.config("state", cd, pd, ensemble=2).__dict__), 8) for cd, pd in (((1088, 64), (64,)), ((64, 1088), (2048,))))
    for call, what in ((lambda: wide.eval_q(None, state, acts), "q_values"), (lambda: wide.sample_best(None, state, eps), "num_candidates")):
        with pytest.raises(_lib.SerlError, match=rf"{what}.*first layer is 1088 wide under wide_widths 1") as e:
            call()
        assert e.value.status == -4, e.value.status      # SERL_ERR_UNSUPPORTED
    assert served.eval_q(None, state, acts).shape == (2, 2, 4) and served.sample_best(None, state, eps)["action"].shape == (2, 4)
