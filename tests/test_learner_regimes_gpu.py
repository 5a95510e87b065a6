"""GPU: the HIP behaviour-cloning learner (csrc/bc.hip) and the reward classifier's train step (csrc/classifier.hip) AWAY from
O.init_params / CO.make_params on noise frames, and at the edges of their row loops (tests/learner_regimes.py, its conditions proved
in tests/test_learner_regimes_cpu.py).

* Trained regime, one step against the fp64 oracles (tests/bc_oracle.py, tests/classifier_train_oracle.py): info scalars at 1e-4
  relative, every gradient leaf (read as the step-1 Adam moments mu = 0.1 g, nu = 0.001 g^2) at 1e-4 of the leaf's maximum, the BC
  head leaves column by column within max(1e-4, 4 x the float32 oracle's error under the same measure), classifier logits at 1e-4 of the
  largest |logit|, the accuracy as an exact float32.
* The clipped columns of the log-std head: gradient exactly 0.0, parameters and moments bit-identical after the step.
* BC inference in the regime: sample_actions at temperature 0, 0.25 and 4 with injected eps against mean + clip(exp(log_std)) sqrt(T) eps,
  get_debug_metrics at the bounds of tests/test_bc_gpu.py.
* The reference's own code in the regime (tests/golden/bc_regime_64.npz, bc_regime_sat_64.npz, classifier_train_regime_one_cam_64.npz),
  with the acceptance rules of tests/test_bc_gpu.py::_check_state (the one-step bc_regime_sat_64: its rule for the moments) and
  tests/test_classifier_train_gpu.py::test_train_loop_equals_the_reference.
* The edge tables: one BC update + sample_actions, one classifier train step per row, at the bounds above; drawn Dropout masks equal
  injected masks bit for bit at 257 rows.

Measured on an MI355X, worst over regime and edge rows: BC info scalars 2.1e-07, gradient leaves (mu) 2.8e-06, head columns 6.0e-07 in the
regime (float32 oracle 9.7e-07, at most 0.006 of the bound) and 8.4e-05 on the edge rows (B1's one near-mean row: float32 oracle 4.4e-05,
0.48 of the bound; every other edge column at most 2.7e-05, 0.27 of it), sample_actions 5.3e-08, log_probs row by row 9.3e-05; classifier logits 1.0e-06,
loss 1.5e-06, gradient leaves (mu) 6.0e-06 in the regime (float32 oracle 5.4e-06) and 8.9e-07 on the edge rows; against the goldens: BC
Adam moments 2.6e-05, classifier loss 6.2e-06.  The nu moments read 1.3e-05 more: float32's 1 - 0.999.  Six arithmetic-only mutations
of bc.hip / classifier.hip that no older test sees each fail tests here: DESIGN.md section 2."""
import numpy as np
import pytest
import torch

from oracle import golden_update as G
import bc_oracle as BO
import classifier_train_oracle as CT
import learner_regimes as LR
from test_bc_cpu import _bernoulli_keep
from test_bc_gpu import _check_state, _close
from test_classifier_train_cpu import bernoulli_host, golden_masks, load_case
from test_learner_regimes_cpu import bc_golden, bc_golden_inputs, cls_golden_inputs

pytestmark = pytest.mark.gpu
TOL = 1e-4


# ---- behaviour cloning ---------------------------------------------------------------------------------------------------------------------
_bc_agent, _bc_batch = LR.bc_agent, LR.bc_batch


def _obs(inp):
    obs = {k: torch.tensor(v[:, None], device="cuda") for k, v in inp["frames"].items()}
    obs["state"] = torch.tensor(inp["state"], device="cuda")
    return obs


def _check_bc_step(what, cfg, agent, info, r64, r32):
    """infos, every gradient leaf through the step-1 moments, and the head leaves column by column against the float32 oracle's error"""
    for k, ref in r64["info"].items():
        e = abs(info[k] - ref) / max(1.0, abs(ref))
        print(f"{what}: info {k} = {info[k]:.7g} (oracle {ref:.7g}), err {e:.2e}")
        assert e < TOL, (what, k, info[k], ref)
    assert agent.state.step == 1
    w_mu = w_nu = 0.0
    for leaf in BO.TRAIN:
        g = r64["grads"][leaf].reshape(-1)
        mu, nu = agent.get("opt/mu", leaf).astype(np.float64), agent.get("opt/nu", leaf).astype(np.float64)
        e_mu, e_nu = LR.rel_err(mu, 0.1 * g), LR.rel_err(nu, 0.001 * g * g)
        w_mu, w_nu = max(w_mu, e_mu), max(w_nu, e_nu)
        assert e_mu < TOL and e_nu < TOL, (what, leaf, e_mu, e_nu)
    print(f"{what}: worst gradient leaf: mu {w_mu:.2e}, nu {w_nu:.2e} (of which 1.3e-5 is float32's 1 - 0.999)")
    bad, worst = [], 0.0
    for leaf in BO.HEAD_LEAVES:
        ref = r64["grads"][leaf]
        e = LR.column_errors(cfg.A, agent.get("opt/mu", leaf).astype(np.float64) / 0.1, ref)
        y = LR.column_errors(cfg.A, r32["grads"][leaf], ref)
        for j in range(cfg.A):
            if np.isnan(y[j]):       # an exactly-zero reference column: _check_clipped_columns
                continue
            bound = max(TOL, 4.0 * y[j])
            worst = max(worst, e[j])
            print(f"{what}: {leaf} column {j}: err {e[j]:.2e}, float32 oracle {y[j]:.2e}, err / bound {e[j] / bound:.3f}")
            if not e[j] <= bound:
                bad.append((leaf, j, e[j], y[j]))
    assert not bad, (what, bad)
    print(f"{what}: worst head column = {worst:.2e}")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_clipped_columns(what, cfg, agent, theta, which):
    """the kernel writes 0.f where the clip binds and sums of zeros are zeros: no tolerance"""
    low, _, high = LR.bc_clip_columns(cfg, which)
    cols = np.concatenate([low, high]).astype(int)
    assert len(cols)
    for leaf in ("actor/logstd/kernel", "actor/logstd/bias"):
        before = np.asarray(theta[leaf], np.float32).reshape(-1, cfg.A)[:, cols]
        for sec in ("opt/mu", "opt/nu"):
            m = agent.get(sec, leaf).reshape(-1, cfg.A)[:, cols]
            assert np.array_equal(_bits(m), _bits(np.zeros_like(before))), (what, sec, leaf, m)
        assert np.array_equal(_bits(agent.get("params", leaf).reshape(-1, cfg.A)[:, cols]), _bits(before)), (what, "params moved", leaf)


@pytest.mark.parametrize("which", LR.BC_SETS)
def test_bc_update_matches_the_oracle_in_the_regime(gpu, which):
    """Measured on an MI355X: see DESIGN.md section 2 ("The BC and classifier learners away from init")"""
    cfg, B = LR.BC_CFG, LR.BC_B
    trunk, theta = LR.bc_theta(cfg, which)
    r64, r32, inp = LR.bc_run(cfg, B, which), LR.bc_run(cfg, B, which, torch.float32), LR.bc_inputs(cfg, B, which)
    agent = _bc_agent(cfg, B, trunk, theta)
    _, info = agent.update(_bc_batch(inp["frames"], inp["state"], inp["action"]), masks=inp["masks"])
    what = f"bc regime {which}"
    _check_bc_step(what, cfg, agent, dict(info), r64, r32)
    _check_clipped_columns(what, cfg, agent, theta, which)


@pytest.mark.parametrize("which", LR.BC_SETS)
def test_bc_inference_matches_the_oracle_in_the_regime(gpu, which):
    cfg, B = LR.BC_CFG, LR.BC_B
    trunk, theta = LR.bc_theta(cfg, which)
    inf = LR.bc_inputs(cfg, B, which)["infer"]
    st = BO.State(cfg, trunk, theta)
    feats = BO.features(trunk, cfg, inf["frames"])
    agent = _bc_agent(cfg, B, trunk, theta)
    obs = _obs(inf)
    mode, mode64 = agent.sample_actions(obs, argmax=True), BO.sample_actions(st, feats, inf["state"]).numpy()
    _close(mode, mode64)
    eps = np.random.default_rng(3).standard_normal((B, cfg.A)).astype(np.float32)
    low, _, high = LR.bc_clip_columns(cfg, which)
    for temp in (0.0, 0.25, 4.0):
        want = BO.sample_actions(st, feats, inf["state"], eps, temp).numpy()
        got = agent.sample_actions(obs, seed=eps, temperature=temp)
        err = np.abs(got - want).max() / max(1.0, np.abs(want).max())
        print(f"bc regime {which}: sample_actions at temperature {temp:g}: err {err:.2e}")
        _close(got, want)
        # the clipped columns by their own scale, as the step from the kernel's own mode: a std_min column moves by 1e-5 sqrt(T) eps,
        # far below the tolerance of the whole array (2e-4 of the step + two float32 spacings of the action it is added to)
        dev, ref = got.astype(np.float64) - mode, want - mode64
        for j in np.concatenate([low, high]).astype(int):
            bound = 2e-4 * np.abs(ref[:, j]).max() + 2 * float(np.spacing(np.float32(np.abs(got[:, j]).max())))
            assert np.abs(dev[:, j] - ref[:, j]).max() <= bound, (temp, j, np.abs(dev[:, j] - ref[:, j]).max(), bound)
    dbg = agent.get_debug_metrics({"observations": obs, "actions": torch.tensor(inf["action"], device="cuda")})
    ref = {k: v.numpy() for k, v in BO.debug_metrics(st, feats, inf["state"], inf["action"]).items()}
    _close(dbg["pi_actions"], ref["pi_actions"])
    _close(dbg["mse"], ref["mse"])
    _close(dbg["log_probs"], ref["log_probs"], 1e-3)
    rows = np.abs(dbg["log_probs"] - ref["log_probs"]) / np.abs(ref["log_probs"])      # ... and row by row: the rows span 1e3 to 1e10
    print(f"bc regime {which}: log_probs row by row, worst {rows.max():.2e}")
    assert rows.max() < 1e-3


@pytest.mark.parametrize("name", [LR.BC_GOLDEN, LR.BC_GOLDEN_SAT])
def test_bc_update_matches_the_reference_golden_in_the_regime(gpu, name):
    """tests/test_bc_gpu.py::test_update_matches_reference_with_injected_masks on bc_regime_64.npz (two updates, no unit at a coarse
    1 - t^2: parameters and moments, _check_state) and on bc_regime_sat_64.npz (one update of the full regime: the moments alone, at
    _check_state's bound -- tests/learner_regimes.py says why the parameter rule is out of float32's reach there)"""
    d, meta, cfg = bc_golden(name)
    trunk, theta, batches, masks = bc_golden_inputs(d, meta, cfg)
    agent = _bc_agent(cfg, meta["B"], trunk, theta)
    agent.state.replace(rng=np.asarray(meta["rng0"], np.uint32))
    for i, (pb, m) in enumerate(zip(batches, masks)):
        _, info = agent.update(_bc_batch({k: v[:, 0] for k, v in pb["frames"].items()}, pb["state"][:, 0], pb["action"]), masks=m)
        ref = d[f"s{i}_info"]
        assert abs(info["actor_loss"] - ref[0]) < TOL * max(1.0, abs(ref[0])), (i, info, ref)
        assert abs(info["mse"] - ref[1]) < TOL * max(1.0, abs(ref[1])), (i, info, ref)
    if name == LR.BC_GOLDEN:
        errs = _check_state(agent, d, meta, meta["steps"])
    else:
        errs = {}
        for sec in ("mu", "nu"):
            for leaf in BO.TRAIN:
                rec = {k.split("|")[2]: d[k] for k in d.files if k.startswith(f"f_{sec}|{leaf}|")}
                errs[(sec, leaf)], _ = G.leaf_compare(f"{sec}/{leaf}", rec, agent.get(f"opt/{sec}", leaf))
                assert errs[(sec, leaf)] < TOL, (sec, leaf, errs[(sec, leaf)])
        assert agent.state.step == meta["final_step"] == 1
    print(f"{name}: worst Adam moment against the reference's run {max(errs.values()):.2e}")
    _check_clipped_columns(name, cfg, agent, theta, "both")


def _edge_which(row):
    return "both" if row[0] in ("B257", "B520") else "max_only"


@pytest.mark.parametrize("row", LR.BC_EDGES, ids=[r[0] for r in LR.BC_EDGES])
def test_bc_edge_shapes_match_the_oracle(gpu, row):
    cfg, B = LR.bc_edge_cfg(row)
    which = _edge_which(row)
    trunk, theta = LR.bc_theta(cfg, which)
    r64, r32, inp = LR.bc_run(cfg, B, which), LR.bc_run(cfg, B, which, torch.float32), LR.bc_inputs(cfg, B, which)
    agent = _bc_agent(cfg, B, trunk, theta)
    what = f"bc edge {row[0]}"
    # inference on other observations, before the step
    inf, st = inp["infer"], r64["state0"]
    feats = BO.features(trunk, cfg, inf["frames"])
    eps = np.random.default_rng(4).standard_normal((B, cfg.A)).astype(np.float32)
    obs = _obs(inf)
    _close(agent.sample_actions(obs, argmax=True), BO.sample_actions(st, feats, inf["state"]).numpy())
    _close(agent.sample_actions(obs, seed=eps, temperature=0.25), BO.sample_actions(st, feats, inf["state"], eps, 0.25).numpy())
    dbg = agent.get_debug_metrics({"observations": obs, "actions": torch.tensor(inf["action"], device="cuda")})
    ref = BO.debug_metrics(st, feats, inf["state"], inf["action"])
    _close(dbg["mse"], ref["mse"].numpy())
    _close(dbg["log_probs"], ref["log_probs"].numpy(), 1e-3)
    # one update
    _, info = agent.update(_bc_batch(inp["frames"], inp["state"], inp["action"]), masks=inp["masks"])
    _check_bc_step(what, cfg, agent, dict(info), r64, r32)
    if len(np.concatenate(LR.bc_clip_columns(cfg, which)[::2])):
        _check_clipped_columns(what, cfg, agent, theta, which)


def test_bc_refuses_an_action_dimension_above_64(gpu):
    from serl_amd import _lib
    cfg, B = LR.bc_edge_cfg(("A65", 1, 7, LR.BC_A_REFUSED, 5))
    with pytest.raises(_lib.SerlError, match=r"status -1: .*act_dim 65"):     # SERL_ERR_INVALID, as serl_bc_create states
        _bc_agent(cfg, B, {}, {})


def test_bc_drawn_masks_equal_injected_masks_beyond_one_trip(gpu):
    row = next(r for r in LR.BC_EDGES if r[0] == "B257")
    cfg, B = LR.bc_edge_cfg(row)
    trunk, theta = LR.bc_theta(cfg, "both")
    inp = LR.bc_inputs(cfg, B, "both")
    batch = _bc_batch(inp["frames"], inp["state"], inp["action"])
    a, b = _bc_agent(cfg, B, trunk, theta), _bc_agent(cfg, B, trunk, theta)
    _, cam_keys = b.update_keys()
    masks = {k: _bernoulli_keep(cam_keys[i], B, 1 - cfg.dropout) for i, k in enumerate(cfg.image_keys)}
    _, ia = a.update(batch)
    _, ib = b.update(batch, masks=masks)
    assert dict(ia) == dict(ib) and np.isfinite(ia["actor_loss"])
    for leaf in BO.TRAIN:
        for sec in ("params", "opt/mu", "opt/nu"):
            assert np.array_equal(_bits(a.get(sec, leaf)), _bits(b.get(sec, leaf))), (sec, leaf)


# ---- reward classifier -----------------------------------------------------------------------------------------------------------------
_classifier = LR.classifier


def _name(keys, leaf):
    return f"enc/{keys.index(leaf.split('/')[1])}/{leaf.split('/', 2)[2]}" if leaf.startswith("enc/") else leaf


def _check_cls_step(what, keys, params, frames, labels, masks, ref):
    from serl_amd.networks.reward_classifier import train_step
    B = len(labels)
    c = _classifier(keys, frames[keys[0]].shape[2], frames[keys[0]].shape[3], params, B)
    scale = max(np.abs(ref["eval"]).max(), np.abs(ref["train"]).max())
    m8 = {k: np.asarray(m, np.uint8) for k, m in masks.items()}
    ev = c.logits(frames).reshape(-1).astype(np.float64)
    tr = c.train_logits(frames, masks=m8).reshape(-1).astype(np.float64)
    e_ev, e_tr = np.abs(ev - ref["eval"]).max() / scale, np.abs(tr - ref["train"]).max() / scale
    print(f"{what}: logits eval {e_ev:.2e}, train {e_tr:.2e} of the largest |logit| = {scale:.1f}")
    assert e_ev < TOL and e_tr < TOL, (what, e_ev, e_tr)
    c, loss, acc = train_step(c, {"data": frames, "labels": labels.reshape(-1, 1)}, None, masks=m8)
    loss, acc = float(loss), float(acc)
    print(f"{what}: loss {loss:.7g} (oracle {ref['loss']:.7g}), err {abs(loss - ref['loss']) / abs(ref['loss']):.2e}; accuracy {acc} ({ref['accuracy']})")
    assert abs(loss - ref["loss"]) < TOL * abs(ref["loss"])
    assert np.float32(acc) == np.float32(ref["accuracy"])
    assert c.step == 1
    w_mu = w_nu = 0.0
    for leaf, g in ref["grads"].items():
        mu, nu = c._get("opt/mu", _name(keys, leaf)).astype(np.float64), c._get("opt/nu", _name(keys, leaf)).astype(np.float64)
        e_mu, e_nu = LR.rel_err(mu, 0.1 * g), LR.rel_err(nu, 0.001 * g * g)
        w_mu, w_nu = max(w_mu, e_mu), max(w_nu, e_nu)
        assert e_mu < TOL and e_nu < TOL, (what, leaf, e_mu, e_nu)
    print(f"{what}: worst gradient leaf: mu {w_mu:.2e}, nu {w_nu:.2e} (of which 1.3e-5 is float32's 1 - 0.999)")
    return c


def test_classifier_train_step_matches_the_oracle_in_the_regime(gpu):
    """Measured on an MI355X: see DESIGN.md section 2 ("The BC and classifier learners away from init")"""
    reg, ref = LR.cls_regime(), LR.cls_run()
    _check_cls_step("classifier regime", LR.CLS_KEYS, reg["params"], reg["frames"], reg["labels"], reg["masks"], ref)


def test_classifier_train_loop_matches_the_reference_golden_in_the_regime(gpu):
    """tests/test_classifier_train_gpu.py::test_train_loop_equals_the_reference on classifier_train_regime_one_cam_64.npz"""
    from serl_amd.networks.reward_classifier import train_step
    d, meta, keys = load_case(LR.CLS_GOLDEN)
    params, cropped, labels = cls_golden_inputs(d, meta, keys)
    lr, steps, B = meta["lr"], meta["epochs"], meta["B"]
    c = _classifier(keys, meta["H"], meta["W"], params, B, lr)
    for e in range(steps):
        masks = {k: m.astype(np.uint8) for k, m in golden_masks(d, e, keys, B).items()}
        c, loss, acc = train_step(c, {"data": {k: v[:, None] for k, v in cropped[e].items()}, "labels": labels.reshape(-1, 1)},
                                  d[f"e{e}_key"], masks=masks)
        ref = float(d[f"e{e}_loss"])
        print(f"{LR.CLS_GOLDEN} epoch {e}: loss {float(loss):.6f} (reference {ref:.6f}), accuracy {float(acc)} ({float(d[f'e{e}_accuracy'])})")
        assert abs(float(loss) - ref) < 1e-4 * abs(ref)
        assert np.float32(float(acc)) == np.float32(d[f"e{e}_accuracy"])
    assert c.step == meta["final_step"]
    for leaf in CT.trainable(keys):
        for sec, name in (("params", "params"), ("mu", "opt/mu"), ("nu", "opt/nu")):
            got = c._get(name, _name(keys, leaf)).astype(np.float64)
            rec = {kind: d[f"f_{sec}|{leaf}|{kind}"] for kind in ("full", "stat", "val") if f"f_{sec}|{leaf}|{kind}" in d.files}
            ref = rec["full"].reshape(-1) if "full" in rec else rec["val"]
            g = got if "full" in rec else got[G._sample_idx(got.size, G._salt(f"{sec}/{leaf}"))]
            diff = np.abs(g - ref)
            if sec == "params":
                assert np.percentile(diff, 99.9) < 1e-4 and diff.max() <= 2 * lr * steps, (leaf, np.percentile(diff, 99.9), diff.max())
            else:
                assert diff.max() <= 1e-4 * np.abs(ref).max() + 1e-30, (sec, leaf, diff.max(), np.abs(ref).max())
    # the frozen trunk: bit-identical, zero moments
    for leaf in (k for k in params if k.startswith("trunk/")):
        assert np.array_equal(c.get(leaf), params[leaf].reshape(-1)), leaf
        assert not np.any(c._get("opt/mu", leaf)) and not np.any(c._get("opt/nu", leaf))


@pytest.mark.parametrize("row", LR.CLS_EDGES, ids=[r[0] for r in LR.CLS_EDGES])
def test_classifier_edge_shapes_match_the_oracle(gpu, row):
    keys, params, frames, labels, masks = LR.cls_edge(row)
    ref = LR.cls_step(params, keys, frames, labels, masks)
    assert np.abs(ref["eval"]).max() > 1.0
    _check_cls_step(f"classifier edge {row[0]}", keys, params, frames, labels, masks, ref)


def test_classifier_drawn_masks_equal_injected_masks_beyond_one_trip(gpu):
    from serl_amd import jaxrng as J
    from serl_amd.networks.reward_classifier import dropout_keys, train_step
    keys, params, frames, labels, _ = LR.cls_edge(next(r for r in LR.CLS_EDGES if r[0] == "B257"))
    B, key = len(labels), J.prngkey(17)
    dk = dropout_keys(key, keys)
    masks = {k: bernoulli_host(dk[i], (B, 4096)).astype(np.uint8) for i, k in enumerate(keys)}
    masks["head"] = bernoulli_host(dk[-1], (B, 256)).astype(np.uint8)
    batch = {"data": frames, "labels": labels.reshape(-1, 1)}
    a, la, aa = train_step(_classifier(keys, LR.EDGE_HW, LR.EDGE_HW, params, B), batch, key)
    b, lb, ab = train_step(_classifier(keys, LR.EDGE_HW, LR.EDGE_HW, params, B), batch, key, masks=masks)
    assert float(la) == float(lb) and float(aa) == float(ab) and np.isfinite(float(la))
    for leaf in a._counts:
        assert np.array_equal(_bits(a.get(leaf)), _bits(b.get(leaf))), leaf
        if not leaf.startswith("trunk/"):
            assert np.array_equal(_bits(a._get("opt/nu", leaf)), _bits(b._get("opt/nu", leaf))), leaf
