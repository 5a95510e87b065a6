"""CPU: Dropout in the critic's and the policy's MLP (networks/mlp.py:27-28; DroQ is the critic's) -- tests/mlp_dropout.py.

* tests/golden/drop_*.npz were produced by tests/golden/make_golden_update_dropout.py from the reference's own update code with a
  positive dropout_rate in the kwargs its factories pass, the MLP masks taken off the stand-in's tape.  The fp64 statement -- the
  oracle's update functions with the recorded masks applied in front of the four LayerNorms of every MLP evaluation -- reproduces
  their infos and final state within F64_TOL of tests/test_reference_update.py, as tests/test_mlp_activations_cpu.py holds its
  fixtures.  That pins placement (bias, then mask, then the statistics of the masked row), scaling and the sharing of one mask
  by all ensemble members, which the GPU tests then compare the kernels with.
* utils.init.mlp_dropout_rates reads the two kwargs as the reference's MLP would.
* The host keys: from the fixture's state.rng, jaxrng.UpdateKeys + flax_make_rng at jaxrng.mlp_dropout_path give every policy
  mask of the run bit for bit; with the stand-in's critic path passed in, every critic mask too -- which pins k_q_target (c),
  k_q_online (split(c)[0], or c with critic_subsample_size None) and k_q_actor (critic_rng)."""
import os

import numpy as np
import pytest
import torch

from oracle import drq_oracle as O
from oracle import golden_update as G
import golden_replay as GR
import mlp_dropout as MD
from serl_amd import jaxrng as J
from serl_amd.utils import init as pinit
from test_reference_update import F64_TOL, _oracle_sections

NAMES = list(MD.GOLDEN)


def _load(name):
    assert os.path.exists(GR.variant_path("drop", name)), f"drop_{name}.npz is not recorded"
    g, meta, z = GR.load_variant("drop", name)
    row = MD.GOLDEN[name]
    assert g["cfg"] == row["cfg"] and g["B"] == row["B"] and int(z["drop_n_sample"]) == row["n_sample"]
    assert (meta["dropout"]["critic"], meta["dropout"]["policy"]) == row["rates"] and meta["prng"] == "threefry"
    assert [s["kind"] for s in g["steps"]] == [s[0] for s in row["sched"]]
    return g, meta, row


@pytest.mark.parametrize("name", NAMES)
def test_fp64_statement_reproduces_the_reference_golden(name):
    g, meta, row = _load(name)
    cfg, rates = g["cfg"], row["rates"]
    for step in g["steps"]:      # every site that draws at these rates is recorded, in the call's shape
        masks = MD.unpack(step["noise"], g["B"], cfg.hidden)
        assert set(masks) == set(MD.sites_of(rates)) & {s for s, _ in MD.site_order(*MD.step_shape(step))}
        if cfg.subsample is None and "q_target" in masks:      # one rng, one scope path: the shared target / online mask
            assert np.array_equal(masks["q_target"], masks["q_online"])
    trunk, theta = GR.initial_leaves(cfg, lambda th, c: {k: np.array(v, np.float32) for k, v in th.items()})
    st = O.TrainState(cfg, trunk, theta, torch.float64)

    def check(i, step, info):
        for k, v in info.items():
            r = step["info"][k]
            assert abs(v - r) <= F64_TOL * max(1.0, abs(r)), (i, k, v, r)
    MD.run_steps(st, g["steps"], rates, on_info=check)
    assert st.step == g["meta"]["final_step"] and O.layer_norm.__module__ == O.__name__
    worst = 0.0
    for sec, tree in _oracle_sections(st).items():
        assert set(g["final"][sec]) == set(tree), sec
        for leaf, t in tree.items():
            e, how = G.leaf_compare(f"{sec}/{leaf}", g["final"][sec][leaf], t.numpy())
            assert e < F64_TOL, (sec, leaf, how, e)
            worst = max(worst, e)
    print(f"drop_{name}: fp64 statement vs reference golden, worst {worst:.1e}")


@pytest.mark.parametrize("name", NAMES[:1])
def test_golden_differs_from_the_run_without_dropout(name):
    """the rate took effect in the reference: the oracle without the masks does not reproduce the first step's critic loss"""
    from oracle import ref_update_runner as RR
    g, _, _ = _load(name)
    trunk, theta = GR.initial_leaves(g["cfg"], lambda th, c: {k: np.array(v, np.float32) for k, v in th.items()})
    st = O.TrainState(g["cfg"], trunk, theta, torch.float64)
    plain = dict(g["steps"][0], noise={k: v for k, v in g["steps"][0]["noise"].items() if not k.startswith("drop_")})
    (info,) = RR.run_steps(st, [plain], torch.float64)
    r = g["steps"][0]["info"]["critic_loss"]
    assert abs(info["critic_loss"] - r) > 1e-3 * abs(r), (info["critic_loss"], r)


def test_statement_places_the_mask_between_bias_and_statistics():
    """x = Dense(x) + b; x = where(keep, x / (1 - rate), 0); LayerNorm's statistics are the masked row's; one mask for all members"""
    cfg = O.Config(image_keys=(), S=10, A=5, hidden=64, ensemble=3)
    th = O.to_torch(O.init_params(cfg, 3)[1], torch.float64)
    th["critic/b1"] = th["critic/b1"] + 0.5      # (a zero bias could not tell "before" from "after")
    enc, a = torch.randn(7, cfg.S, dtype=torch.float64), torch.randn(7, cfg.A, dtype=torch.float64)
    rng = np.random.default_rng(0)
    m = (rng.random((2, 7, 64)) < 0.7).astype(np.uint8)
    with MD.oracle_dropout((0.3, 0.0), [("q_online", 0, m[0]), ("q_online", 1, m[1])]) as seen:
        q = O.critic_forward(th, cfg, enc, a)
    x = torch.cat([enc, a], -1)
    h = torch.einsum("bi,eio->ebo", x, th["critic/w1"]) + th["critic/b1"][:, None, :]
    h = h * torch.tensor(m[0], dtype=torch.float64) / 0.7
    assert torch.allclose(seen[0][2], h, rtol=0, atol=1e-15) and (seen[0][2][:, m[0] == 0] == 0).all()
    h = torch.tanh(O.layer_norm(h, th["critic/ln1/scale"][:, None, :], th["critic/ln1/bias"][:, None, :]))
    h = torch.einsum("ebi,eio->ebo", h, th["critic/w2"]) + th["critic/b2"][:, None, :]
    h = torch.tanh(O.layer_norm(h * torch.tensor(m[1], dtype=torch.float64) / 0.7, th["critic/ln2/scale"][:, None, :], th["critic/ln2/bias"][:, None, :]))
    want = torch.einsum("ebi,eio->ebo", h, th["critic/head/kernel"]).squeeze(-1) + th["critic/head/bias"][:, None]
    assert torch.allclose(q, want, rtol=0, atol=1e-14)
    with MD.oracle_dropout((0.0, 0.0), []):      # rate 0: the oracle itself
        assert torch.equal(O.critic_forward(th, cfg, enc, a), O.critic_forward(th, cfg, enc, a))


# ---- reading the kwargs ----------------------------------------------------------------------------------------------------------
def test_mlp_dropout_rates_reads_what_the_reference_reads():
    assert pinit.mlp_dropout_rates(None, None) == pinit.mlp_dropout_rates({}, {}) == (0.0, 0.0)
    assert pinit.mlp_dropout_rates({"dropout_rate": None}, {"dropout_rate": 0}) == (0.0, 0.0)
    assert pinit.mlp_dropout_rates({"dropout_rate": -0.5}, {"dropout_rate": 0.0}) == (0.0, 0.0)      # mlp.py:27: `> 0`
    assert pinit.mlp_dropout_rates({"dropout_rate": 0.1}, None) == (0.1, 0.0)
    assert pinit.mlp_dropout_rates(None, {"dropout_rate": np.float32(0.25)}) == (0.0, 0.25)
    assert pinit.mlp_dropout_rates({"dropout_rate": 0.01, "activations": "swish"}, {"dropout_rate": 0.99}) == (0.01, 0.99)
    # with the switch on, mlp_activations leaves the rates alone; without it a positive rate is refused as it always was
    assert pinit.mlp_activations({"dropout_rate": 0.1}, {"dropout_rate": 0.05, "activations": "relu"}, mlp_dropout=True) == ("tanh", "relu")
    with pytest.raises(NotImplementedError, match="critic_network_kwargs: dropout_rate=0.1") as e:
        pinit.mlp_activations({"dropout_rate": 0.1}, None)
    assert "mlp_dropout=True" in str(e.value)


@pytest.mark.parametrize("create", ["create_states", "create_drq"])
def test_create_reads_the_rates_only_with_the_switch(create):
    """no device is touched: without mlp_dropout=True a positive rate is refused from the arguments alone, naming the switch; with
    it a rate the rows cannot serve is refused by mlp_dropout_rates"""
    from test_mlp_widths_cpu import _create_drq, _create_states
    fn = {"create_states": _create_states, "create_drq": _create_drq}[create]
    with pytest.raises(NotImplementedError, match="dropout_rate=0.1") as e:
        fn(critic_network_kwargs={"dropout_rate": 0.1})
    assert "mlp_dropout=True" in str(e.value)
    with pytest.raises(NotImplementedError, match="dropout_rate=1.5") as e:
        fn(policy_network_kwargs={"dropout_rate": 1.5}, mlp_dropout=True)
    assert "served: dropout_rate None or a number below 1" in str(e.value)


@pytest.mark.parametrize("which", ["critic_network_kwargs", "policy_network_kwargs"])
@pytest.mark.parametrize("rate", [1.0, 1, 2.5, "0.1", True, [0.1], float("nan")], ids=str)
def test_mlp_dropout_rates_refuses_what_is_not_served(which, rate):
    args = {"critic_network_kwargs": {}, "policy_network_kwargs": {}, which: {"dropout_rate": rate}}
    with pytest.raises(NotImplementedError, match=which) as e:
        pinit.mlp_dropout_rates(**args)
    assert "served: dropout_rate None or a number below 1" in str(e.value) and repr(rate) in str(e.value)


# ---- the host keys ---------------------------------------------------------------------------------------------------------------
def _bernoulli(key, keep, rows, h):
    """jax.random.bernoulli(key, keep, (rows, h)) from the library's host bits: uniform(bits) < keep in float32"""
    bits = J.random_bits(key, rows * h)
    u = ((bits >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1.0)
    return (u < np.float32(keep)).astype(np.uint8).reshape(rows, h)


def _call_keys(cfg, step, rng, subsample_none):
    kind, n_critic, nets = MD.step_shape(step)
    if kind == "update":
        act = bool(set(nets) & {"actor", "temperature"})
        return J.UpdateKeys(rng, False, n_critic, act, n_critic == 1 and act, subsample_none)
    return J.UpdateKeys(rng, not cfg.state_only, n_critic, kind == "high_utd", False, subsample_none)


def _site_rngs(keys, step):
    kind, n_critic, nets = MD.step_shape(step)
    out = {}
    if n_critic:
        out.update(pi_next=keys.k_next_action, q_target=keys.k_q_target, q_online=keys.k_q_online)
    if keys.has_actor_temp:
        out.update(pi=keys.k_policy, q_actor=keys.k_q_actor, pi_temp=keys.k_temp)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_host_keys_reproduce_the_recorded_masks(name):
    g, meta, row = _load(name)
    cfg, B, rates = g["cfg"], g["B"], row["rates"]
    rate = {"critic": rates[0], "policy": rates[1]}
    assert meta["dropout"]["standin_critic_path"] == list(MD.standin_dropout_path("critic", 0, cfg.state_only))
    rng = np.array(meta["rng0"], np.uint32)
    n = 0
    for step in g["steps"]:
        keys = _call_keys(cfg, step, rng, cfg.subsample is None)
        rngs = _site_rngs(keys, step)
        masks = MD.unpack(step["noise"], B, cfg.hidden)
        _, n_critic, _ = MD.step_shape(step)
        mb = B // max(n_critic, 1)
        for site, m in masks.items():
            net = MD.MLP_SITE_NETWORK[site]
            # the policy's path is the library's own; the critic's is the stand-in's, passed as data
            path = (lambda l: J.mlp_dropout_path("policy", l)) if net == "policy" else (lambda l: MD.standin_dropout_path("critic", l, cfg.state_only))
            for layer in (0, 1):
                if site in MD.MLP_CRITIC_LOSS_SITES:
                    got = np.concatenate([_bernoulli(J.flax_make_rng(k, path(layer), 1), 1 - rate[net], mb, cfg.hidden) for k in rngs[site]])
                else:
                    got = _bernoulli(J.flax_make_rng(rngs[site], path(layer), 1), 1 - rate[net], B, cfg.hidden)
                assert np.array_equal(got, m[layer]), (site, layer)
                n += 1
        if cfg.subsample is None and n_critic:
            assert all(np.array_equal(a, b) for a, b in zip(keys.k_q_target, keys.k_q_online))
        elif n_critic:
            assert all(np.array_equal(J.split(a)[0], b) for a, b in zip(keys.k_q_target, keys.k_q_online))
        rng = keys.rng_out
    assert [int(v) for v in rng] == meta["rng_final"] and n >= 6
    print(f"drop_{name}: {n} masks reproduced from state.rng")


def test_keys_without_dropout_are_the_parents():
    rng = J.prngkey(7)
    for args in ((True, 3, True, False), (False, 1, True, True), (False, 0, True, False), (True, 40, True, False)):
        old = J.UpdateKeys(rng, *args)
        assert not hasattr(old, "k_q_target") and not hasattr(old, "k_q_actor")
        for sub_none in (False, True):
            new = J.UpdateKeys(rng, *args, sub_none)
            for f in ("rng_out", "k_policy", "k_sample", "k_temp"):
                assert np.array_equal(getattr(old, f), getattr(new, f)), f
            for f in ("k_next_action", "k_subsample"):
                assert len(getattr(old, f)) == len(getattr(new, f)) == args[1]
                assert all(np.array_equal(a, b) for a, b in zip(getattr(old, f), getattr(new, f))), f
            assert len(new.k_q_target) == len(new.k_q_online) == args[1]
            for c, k_na, k_on, k_sub in zip(new.k_q_target, new.k_next_action, new.k_q_online, new.k_subsample):
                # c, k_next_action = split(r_critic); online rng, k_subsample = split(c) -- or the online rng is c itself
                s = J.split(c)
                assert np.array_equal(s[1], k_sub) and np.array_equal(k_on, c if sub_none else s[0]) and not np.array_equal(c, k_na)


def test_mlp_dropout_path_states_the_scope_once():
    assert J.mlp_dropout_path("policy", 0) == ("modules_actor", "network", "Dropout_0")
    assert J.mlp_dropout_path("critic", 1) == ("modules_critic", "network", "Dropout_1")
    with pytest.raises(KeyError):
        J.mlp_dropout_path("encoder", 0)


def test_call_noise_builds_keys_for_the_sites_that_draw():
    """CallNoise on a duck-typed core: the "keys" form names exactly the sites whose network drops, critic-loss sites per update"""
    from serl_amd.call_noise import CallNoise

    class Cfg:
        critic_subsample_size, ensemble, n_cam, encoder_type, hidden = 2, 10, 0, 1, 256

    class Core:
        cfg, critic_dropout, policy_dropout = Cfg(), 0.01, 0.0
    cn = CallNoise(Core(), (), {})
    keys = J.UpdateKeys(J.prngkey(3), False, 2, True, False, False)
    noise = cn.build(keys, 8, "keys")
    assert {k for k in noise if k.startswith("drop_")} == {"drop_key_q_target", "drop_key_q_online", "drop_key_q_actor"}
    assert noise["drop_key_q_target"].shape == (2, 2, 2) and noise["drop_key_q_actor"].shape == (2, 2)
    assert np.array_equal(noise["drop_key_q_online"][1, 1], J.flax_make_rng(keys.k_q_online[1], J.mlp_dropout_path("critic", 1), 1))
    Core.critic_dropout, Core.policy_dropout = 0.0, 0.0
    plain = CallNoise(Core(), (), {}).build(J.UpdateKeys(J.prngkey(3), False, 2, True), 8, "keys")
    assert not any(k.startswith("drop_") for k in plain)
