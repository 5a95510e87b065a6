"""GPU: MLP Dropout at every served shape (mlp_dropout="any", serl_agent_opts.dropout_any) under the whole update chain, on the case
table of tests/droq_shapes.py, against the fp64 oracle with injected u8 masks at TOL = 1e-4 (tests/test_mlp_shapes_gpu.py's).
Without the switch every case fails when its agent is made (NotImplementedError from NetSpec.check)."""
import numpy as np
import pytest
import torch

from oracle import drq_oracle as O
from serl_amd import jaxrng as J
import agent_helpers as AH
import droq_shapes as DS
import mlp_plain as MP
import mlp_ragged as MR
from test_agent_gpu import _compare_state
from test_chain_fusion_gpu import _assert_state_bits, _bits_equal, _launches
from test_mlp_widths_gpu import _Figures, _info

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _general_oracle():
    with DS.installed():
        yield


def _run(core, run, call, extra=None):
    cfg = run["cfg"]
    db, dn = AH.batch_to_device(cfg, run["batch"]), {**AH.noise_to_device(cfg, run["noise"]), **(DS.device_noise(run["masks"]) if extra is None else extra)}
    core.update_critics(db, dn) if call == "critics" else core.update_high_utd(db, call[1], dn)
    return core


@pytest.mark.parametrize("name", list(DS.CASES))
def test_updates_match_the_oracle_in_both_schedules(gpu, name):
    """fused == un-fused bit for bit; info scalars, q, target_q, every gradient leaf (pads asserted zero) and the state after the
    step against the fp64 oracle with the same masks; the pad invariant after the updates; relu pre-activations off the kink"""
    for call in DS.calls_of(name):
        run = DS.oracle_run(name, call)
        cfg, B, aux, crit = run["cfg"], run["B"], run["aux"], call == "critics"
        assert all(m >= MP.RELU_MARGIN for m in run["relu"]) and bool(run["relu"]) == ("relu" in (cfg.critic_activation, cfg.policy_activation))
        cores = [_run(DS.make_core(cfg, B, run["rates"], run["leaves"], fuse=f), run, call) for f in (True, False)]
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


def test_a_wide_row_alone_has_the_bits_it_has_among_65(gpu):
    """the one-row case's update_critics is row 0 of the 65-row case's (DS.oracle_run): Q and the first layer's normalised row"""
    got = []
    for name in ("wide", "wide_one_row"):
        run = DS.oracle_run(name, "critics")
        core, B, E = _run(DS.make_core(run["cfg"], run["B"], run["rates"], run["leaves"]), run, "critics"), run["B"], run["cfg"].ensemble
        got.append((core.debug("q", E * B).reshape(E, B)[:, 0], core.debug("mlp_xhat/crit_/1", E * B * 1088).reshape(E, B, 1088)[:, 0]))
    assert _bits_equal(got[0][0], got[1][0]) and _bits_equal(got[0][1], got[1][1])


@pytest.mark.parametrize("name,layers", [("ragged", ((65, 128), (127, 128))), ("wide", ((64, 64), (1088, 1088)))])
def test_backward_restates_the_forward_from_the_key_and_from_the_hash(gpu, name, layers):
    """the policy's backward runs last: dpre is exactly 0 where the forward dropped and nowhere else among the true columns, never
    in a pad.  From the key: the host's bernoulli over (rows, Nt).  From the hash (192 rows: 2.1e5 elements at 1088): every dropped
    column of a LayerNorm row holds one xhat value, and the kept fraction is keep within 4 sigma of Binomial(n, keep)."""
    run = DS.oracle_run(name, ("high_utd", 5))
    cfg, keep = run["cfg"], np.float32(1.0 - run["rates"][1])
    keys = {"drop_key_" + s: (J.split(J.prngkey(9 + i), 5 * len(d)).reshape(5, len(d), 2) if s in ("pi_next", "q_target", "q_online")
                              else J.split(J.prngkey(9 + i), len(d)))
            for i, (s, d) in enumerate((s, cfg.policy_dims if s.startswith("pi") else cfg.critic_dims) for s in DS.MD.MLP_SITES)}
    big = dict(run, B=192, batch=AH.synth_batch(cfg, 192, seed=5), noise=O.make_noise(cfg, 192, seed=6, utd_ratio=2))
    for r, call, noise in ((run, ("high_utd", 5), keys), (big, ("high_utd", 2), {})):
        B = r["B"]
        core = _run(DS.make_core(cfg, B, r["rates"], r["leaves"]), r, call, extra=noise)
        for l, (d, dp) in enumerate(layers):
            dpre = core.debug(f"mlp_dpre/{l + 1}", B * dp).reshape(B, dp)
            assert not dpre[:, d:].any(), (name, l)
            if noise:
                bits = J.random_bits(keys["drop_key_pi"][l], B * d).astype(np.uint32)
                want = ((((bits >> 9) | 0x3F800000).view(np.float32) - np.float32(1.0)) < keep).reshape(B, d)
                assert np.array_equal(dpre[:, :d] != 0, want), (name, l)
                continue
            xhat, dropped = core.debug(f"mlp_xhat/pol__/{l + 1}", B * dp).reshape(B, dp)[:, :d], dpre[:, :d] == 0
            assert all(np.unique(xhat[i][dropped[i]]).size <= 1 for i in range(B)), (name, l)
            n, sigma = dropped.size, np.sqrt(keep * (1.0 - keep) / dropped.size)
            assert abs((n - dropped.sum()) / n - keep) <= 4.0 * sigma, (name, l, n, dropped.sum())


def _two_calls(agent, seed, masks=None):
    """update and update_high_utd(2) on 8 rows with injected noise (masks None: random ones by the agent's widths) -> launches"""
    if masks is None:
        rng = np.random.default_rng(seed)
        masks = {"drop_mask_" + s: [torch.tensor((rng.random((8, d)) < 0.9).astype(np.uint8), device="cuda")
                                    for d in (agent.core.policy_dims if s.startswith("pi") else agent.core.critic_dims)] for s in DS.MD.MLP_SITES}
    from test_mlp_widths_gpu import _flat_batch
    torch.cuda.synchronize()
    l0 = _launches()
    for it, call in enumerate((agent.update, lambda b, **k: agent.update_high_utd(b, utd_ratio=2, **k))):
        cfg = O.Config(image_keys=(), S=10, A=4, ensemble=2, discount=0.99)
        noise = {**AH.noise_to_device(cfg, O.make_noise(cfg, 8, seed=seed + it, utd_ratio=1 + it)), **masks}
        call(_flat_batch(10, 4, 8, seed + it), noise=noise)
    torch.cuda.synchronize()
    return _launches() - l0


def test_256_256_through_any_is_the_agent_of_true_and_a_checkpoint_of_the_shapes_case_restores(gpu, tmp_path):
    from serl_amd.utils.checkpoint import restore_checkpoint, save_checkpoint
    import mlp_shapes as MS
    kw = lambda dims, r: MS.mlp_kwargs(dims, dropout_rate=r)      # noqa: E731
    rng = np.random.default_rng(1)
    masks = {"drop_mask_" + s: torch.tensor((rng.random((2, 8, 256)) < 0.9).astype(np.uint8), device="cuda") for s in DS.MD.MLP_SITES}
    a_any, a_true = (MS.sac_agent((256, 256), (256, 256), seed=3, B=8, critic_ensemble_size=2, mlp_dropout=m,
                                  critic_network_kwargs=kw((256, 256), 0.1), policy_network_kwargs=kw((256, 256), 0.1)) for m in ("any", True))
    assert a_any.core.spec.dropout_any and not a_true.core.spec.dropout_any and a_any.core.L.serl_agent_dropout_any(a_any.core._h) == 1
    assert _two_calls(a_any, 50, masks) == _two_calls(a_true, 50, masks)
    want = MR.all_bits(a_true.core)
    assert all(_bits_equal(v, want[k]) for k, v in MR.all_bits(a_any.core).items()) and a_any.core.read_info() == a_true.core.read_info()
    shapes = dict(critic_network_kwargs=kw((128, 64, 192), 0.1), policy_network_kwargs=kw((64,), 0.2))
    agent, again = (MS.sac_agent((128, 64, 192), (64,), seed=s, B=8, critic_ensemble_size=2, mlp_dropout="any", **shapes) for s in (7, 2))
    assert agent.config["dropout_any"] is True
    _two_calls(agent, 60)
    save_checkpoint(str(tmp_path / "droq"), agent, step=agent.state.step)
    restore_checkpoint(str(tmp_path / "droq"), again, restore_rng=True)
    for a in (agent, again):
        _two_calls(a, 70)
    want = MR.all_bits(agent.core)
    assert all(_bits_equal(v, want[k]) for k, v in MR.all_bits(again.core).items())
