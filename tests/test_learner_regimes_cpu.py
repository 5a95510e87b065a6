"""CPU: the oracles and the regimes of tests/learner_regimes.py, proved without the code under test.

* tests/bc_oracle.py (the whole BC update from the frames on, torch autograd) reproduces the reference's own BCAgent as recorded in
  tests/golden/bc_{64,one_cam,84,64_seq}.npz and agrees with tests/test_bc_cpu.py::_np_bc (the head and MLP, by hand), at 1e-9.
* It reproduces tests/golden/bc_regime_64.npz and bc_regime_sat_64.npz, and tests/classifier_train_oracle.py reproduces
  tests/golden/classifier_train_regime_one_cam_64.npz: the reference's unmodified BCAgent / BinaryClassifier + training loop under
  oracle/jaxshim on the regime parameters and batches (tests/golden/make_golden_bc.py, make_golden_classifier_train.py), at 1e-9
  (measured: 1.9e-15, 1.9e-15, 1.1e-14), the reference's exactly-zero Adam moments of the clipped log-std columns included.
* The regime conditions, on the fp64 oracles alone.  Measured: BC log_std at least 1.20 from both clip bounds; 25.0% / 25.4% of the
  units of the two tanh layers exactly +-1 in float32 and 21.9% / 23.0% with a coarse 1 - t^2, in every row; classifier eval and train
  logits from 0.90 to 92 in magnitude, min |eval logit| 0.898, accuracy 11/16.
* Attainability: the float32 oracles (float32 throughout, frozen trunk included) against the fp64 ones under the measures of the GPU
  tests, bound 2e-5 as tests/test_trained_regime_cpu.py.  Measured: BC infos 7.3e-8, gradient leaves 9.4e-7, head columns 9.7e-7;
  classifier loss 1.5e-6, logits 2.5e-6, gradient leaves 5.4e-6 (the case was softened twice to get there: tests/learner_regimes.py).
* The edge tables hold every class they claim."""
import json
import math
import os
import zlib

import numpy as np
import pytest
import torch

from oracle import drq_oracle as O
from oracle import golden_update as G
from oracle.ref_update_runner import synth_packed_batch
import bc_oracle as BO
import classifier_train_oracle as CT
import learner_regimes as LR
from test_bc_cpu import _np_bc
from test_classifier_train_cpu import golden_masks, load_case

HERE = os.path.dirname(os.path.abspath(__file__))
F64_TOL, F32_YARDSTICK = 1e-9, 2e-5


# ---- the BC oracle against the reference's recorded runs -----------------------------------------------------------------------------
def bc_golden(name):
    d = np.load(os.path.join(HERE, "golden", f"{name}.npz"))
    meta = json.loads(str(d["meta"]))
    return d, meta, G.cfg_from_dict(meta["cfg"])


def bc_golden_inputs(d, meta, cfg):
    """-> (trunk, theta, [packed batch of step i], its [keep-masks]) as the recipe built them"""
    trunk, theta = O.init_params(cfg, meta["param_seed"])
    bt = None
    if "regime" in meta:
        rg = meta["regime"]
        assert rg["transform"] == "bc_trained_like" and rg["seed"] == LR.BC_SEED and rg["batch_seed"] == LR.BC_BATCH_SEED
        assert rg["which"] == "both" and tuple(rg["sat_bias"]) in LR.BC_GOLDEN_SAT_BIASES.values()
        theta = LR.bc_golden_theta_transform(tuple(rg["sat_bias"]))(theta, cfg)
        bt = LR.bc_golden_batch_transform(cfg, meta["param_seed"], tuple(rg["sat_bias"]))
    batches, masks = [], []
    for i in range(meta["steps"]):
        pb = synth_packed_batch(cfg, meta["B"], meta["batch_seed"] + i)
        pb = bt(pb, i) if bt else pb
        for k, v in pb["frames"].items():
            assert np.uint32(zlib.crc32(v.tobytes())) == d[f"s{i}_crc_{k}"]
        batches.append(pb)
        masks.append({k: np.unpackbits(d[f"s{i}_mask_{k}"])[:meta["B"] * 4096].reshape(meta["B"], 4096) for k in cfg.image_keys})
    return trunk, theta, batches, masks


def _replay_bc(name):
    d, meta, cfg = bc_golden(name)
    trunk, theta, batches, masks = bc_golden_inputs(d, meta, cfg)
    st = BO.State(cfg, trunk, theta)
    first = None
    for i, (pb, m) in enumerate(zip(batches, masks)):
        feats = BO.features(trunk, cfg, {k: v[:, 0] for k, v in pb["frames"].items()})
        info, grads, aux = BO.update(st, feats, pb["state"][:, 0], pb["action"], m)
        first = first or (grads, aux, pb)
        ref = d[f"s{i}_info"]
        assert abs(info["actor_loss"] - ref[0]) < F64_TOL * max(1.0, abs(ref[0])), (i, info, ref)
        assert abs(info["mse"] - ref[1]) < F64_TOL * max(1.0, abs(ref[1])), (i, info, ref)
    assert st.step == meta["final_step"]
    worst = 0.0
    for leaf in BO.TRAIN:
        for sec, t in (("params", st.params), ("mu", st.mu), ("nu", st.nu)):
            rec = {k.split("|")[2]: d[k] for k in d.files if k.startswith(f"f_{sec}|{leaf}|")}
            err, how = G.leaf_compare(f"{sec}/{leaf}", rec, t[leaf].numpy())
            assert err < F64_TOL, (sec, leaf, err, how)
            worst = max(worst, err)
    print(f"{name}: bc_oracle vs the reference's run, worst leaf {worst:.1e}")
    return d, meta, cfg, theta, first


@pytest.mark.parametrize("name", ["bc_64", "bc_one_cam", "bc_84", "bc_64_seq"])
def test_bc_oracle_reproduces_the_reference_goldens(name):
    d, meta, cfg, theta, (grads, aux, pb) = _replay_bc(name)
    # ... and the hand-written head / MLP of tests/test_bc_cpu.py, from this oracle's own encoder output
    if "enc0" in d.files:
        assert np.abs(aux["enc"].numpy() - d["enc0"]).max() < F64_TOL
    loss, mse, g = _np_bc(theta, aux["enc"].numpy(), pb["action"].astype(np.float64))
    for leaf, ref in g.items():
        assert LR.rel_err(grads[leaf].numpy(), ref) < F64_TOL, leaf


@pytest.mark.parametrize("name,steps", [(LR.BC_GOLDEN, 2), (LR.BC_GOLDEN_SAT, 1)])
def test_bc_oracle_reproduces_the_regime_golden(name, steps):
    d, meta, cfg, theta, (grads, aux, pb) = _replay_bc(name)
    assert meta["steps"] == steps and meta["B"] == LR.BC_B and cfg.A == 5 and cfg.n_cam == 2 and (cfg.H, cfg.W) == (64, 64)
    assert tuple(meta["regime"]["sat_bias"]) == LR.BC_GOLDEN_SAT_BIASES[name]
    # hidden units at exactly +-1 in float32: none in the two-step golden, a quarter in the one-step one
    sat = min((np.abs(aux[h].numpy().astype(np.float32)) == 1.0).mean(axis=1).min() for h in ("h1", "h2"))
    assert sat == 0.0 if name == LR.BC_GOLDEN else sat >= LR.SAT_SHARE, sat
    _, _, g = _np_bc(theta, aux["enc"].numpy(), pb["action"].astype(np.float64))
    for leaf, ref in g.items():
        assert LR.rel_err(grads[leaf].numpy(), ref) < F64_TOL, leaf
    # the recorded run is in the regime: whole columns on either side of the clip, in every row of the first update
    low, mid, high = LR.bc_clip_columns(cfg, "both")
    ls = aux["log_std"].numpy()
    assert len(low) and len(high) and (ls[:, low] < math.log(cfg.std_min)).all() and (ls[:, high] > math.log(cfg.std_max)).all()
    # the reference's own Adam moments of the clipped log_std columns are exactly zero after every update
    for sec in ("mu", "nu"):
        b = d[f"f_{sec}|actor/logstd/bias|full"]
        k = d[f"f_{sec}|actor/logstd/kernel|full"].reshape(-1, cfg.A)
        cl = np.concatenate([low, high])
        assert (b[cl] == 0.0).all() and (b[mid] != 0.0).all() and (k[:, cl] == 0.0).all() and (k[:, mid] != 0.0).any(), sec
    assert d["s0_info"][0] > 1e9      # the std_min columns: (a - mean)^2 / (2 * 1e-10)


# ---- the classifier oracle against the reference's recorded loop in the regime -------------------------------------------------------
def cls_golden_inputs(d, meta, keys):
    """-> (params, [cropped frames {k: u8 [B, H, W, 3]} of epoch e], labels) as the recipe built them"""
    from serl_amd import jaxrng as J
    B, H, W = meta["B"], meta["H"], meta["W"]
    assert meta["regime"]["params"] == "cls_golden_params" and tuple(meta["regime"]["targets"]) == LR.CLS_GOLDEN_TARGETS
    frames = LR.cls_golden_frames(keys, H, W, B, meta["epochs"])
    cropped = [{k: CT.host_crop(v[:, 0], J.crop_offsets(d[f"e{e}_crop_key"], B, padding=4)) for k, v in frames[e].items()}
               for e in range(meta["epochs"])]
    assert np.array_equal(cropped[0][keys[0]][:2], d[f"e0_cropped_{keys[0]}"][:, 0])
    return LR.cls_golden_params(keys, H, W, meta["param_seed"], cropped), cropped, LR.cls_labels(B)


def test_classifier_oracle_reproduces_the_regime_golden():
    d, meta, keys = load_case(LR.CLS_GOLDEN)
    assert meta["epochs"] == 2 and meta["B"] == LR.CLS_GOLDEN_B and (meta["H"], meta["W"]) == (64, 64) and len(keys) == 1
    params, cropped, labels = cls_golden_inputs(d, meta, keys)
    st = CT.State(params, keys, lr=meta["lr"])
    for e in range(meta["epochs"]):
        feats = CT.features(params, keys, cropped[e])
        loss, acc, ev, _ = CT.train_step(st, feats, labels, golden_masks(d, e, keys, meta["B"]))
        assert abs(loss - float(d[f"e{e}_loss"])) < F64_TOL * max(1.0, abs(loss)), (e, loss, float(d[f"e{e}_loss"]))
        assert acc == float(d[f"e{e}_accuracy"]) == 4.0 / 6.0
        assert np.abs(ev - d[f"e{e}_logits_eval"]).max() < F64_TOL * np.abs(ev).max()
        # the recorded run is in the regime: its own eval logits start on the targets the head was fitted to (one Adam step of 1e-4 on
        # every weight of the 4096-wide layers then moves them by tens: epoch 1 runs at |logit| from 36 to 124)
        rec = d[f"e{e}_logits_eval"].reshape(-1)
        assert np.abs(rec - np.array(LR.CLS_GOLDEN_TARGETS)).max() < 0.1 if e == 0 else np.abs(rec).min() > 17, rec
    assert st.step == meta["final_step"]
    worst = 0.0
    for leaf in CT.trainable(keys):
        for sec, v in (("params", st.params[leaf]), ("mu", st.mu[leaf]), ("nu", st.nu[leaf])):
            rec = {kind: d[f"f_{sec}|{leaf}|{kind}"] for kind in ("full", "stat", "val") if f"f_{sec}|{leaf}|{kind}" in d.files}
            err, how = G.leaf_compare(f"{sec}/{leaf}", rec, v)
            assert err < F64_TOL, (sec, leaf, err, how)
            worst = max(worst, err)
    print(f"classifier_train_{LR.CLS_GOLDEN}: classifier_train_oracle vs the reference's loop, worst leaf {worst:.1e}")


# ---- the regime conditions: inputs of tests/test_learner_regimes_gpu.py, not measurements of the code under test --------------------------
@pytest.mark.parametrize("which", LR.BC_SETS)
def test_the_bc_recipe_reaches_the_regime(which):
    cfg, B = LR.BC_CFG, LR.BC_B
    r, r32, inp = LR.bc_run(cfg, B, which), LR.bc_run(cfg, B, which, torch.float32), LR.bc_inputs(cfg, B, which)
    lo_b, hi_b = math.log(cfg.std_min), math.log(cfg.std_max)
    low, mid, high = LR.bc_clip_columns(cfg, which)
    assert len(high) >= 1 and len(mid) >= 2 and (len(low) >= 1) == (which == "both")
    ls = r["aux"]["log_std"]
    assert ls.shape == (B, cfg.A)
    assert (ls[:, low] < lo_b).all() and (ls[:, high] > hi_b).all() and ((ls[:, mid] > lo_b) & (ls[:, mid] < hi_b)).all()
    margin = min(float(np.abs(ls - lo_b).min()), float(np.abs(ls - hi_b).min()))
    assert margin >= 0.5, margin
    for h in ("h1", "h2"):       # shares of the hidden units, in the worst row, as float32 sees them
        t = r32["aux"][h].astype(np.float32)
        om = np.float32(1.0) - t * t
        sat, coarse = (np.abs(t) == 1.0).mean(axis=1).min(), ((om > 0) & (om < 1e-4)).mean(axis=1).min()
        print(f"bc {which}: {h}: exactly +-1 in {sat:.1%} of the units, coarse 1 - t^2 in {coarse:.1%} (worst row); min |log_std - log(bound)| = {margin:.2f}")
        assert sat >= LR.SAT_SHARE and coarse >= LR.COARSE_SHARE, (h, sat, coarse)
        assert (np.abs(r["aux"][h]) < 0.9).mean() >= 0.3      # and a good part of the rest is not saturated
    mean = r["aux"]["mean"]
    assert (np.abs(mean) > 2.0).any() and (np.abs(mean) < 0.5).any()
    gb, gk = r["grads"]["actor/logstd/bias"], r["grads"]["actor/logstd/kernel"]
    cl = np.concatenate([low, high])
    assert (gb[cl] == 0.0).all() and (gk[:, cl] == 0.0).all() and (gb[mid] != 0.0).all()
    # the batch is what harden_bc_batch promises
    a, d = inp["action"], inp["action"] - mean.astype(np.float32)
    kind = np.add.outer(np.arange(B), np.arange(cfg.A)) % 4
    assert (np.abs(a[kind == 0]) == 1.0).all() and (np.abs(d[kind == 1]) <= 1.01e-3).all() and (np.abs(d[kind == 2]) >= 2.99).all()
    assert np.abs(inp["state"]).max() > 20
    sc = LR.bc_theta(cfg, which)[1]["enc/proprio/ln/scale"]
    assert (sc < 0).any() and (sc > 0).any()


def _bands(l):
    a = np.abs(l)
    return {"below 1": a < 1, "5 to 15": (a >= 5) & (a <= 15), "above 17": (a > 17) & (a <= 90), "beyond 90": a > 90}


def test_the_classifier_recipe_reaches_the_regime():
    r, reg = LR.cls_run(), LR.cls_regime()
    y = reg["labels"]
    for what in ("eval", "train"):
        l = r[what]
        assert (l > 0).any() and (l < 0).any()
        for band, sel in _bands(l).items():
            hit = (l[sel] >= 0) == (y[sel] == 1)
            assert sel.any() and hit.any() and (~hit).any(), (what, band, l[sel], y[sel])
        assert (l > 90).any() and (l < -90).any()
        print(f"classifier regime: {what} logits |l| from {np.abs(l).min():.3f} to {np.abs(l).max():.1f}")
    assert np.abs(r["eval"]).min() >= 1e-3
    assert np.abs(r["eval"] - np.array(LR.CLS_TARGETS)).max() < 0.1 and np.abs(r["train"] - np.array(LR.CLS_TRAIN_TARGETS)).max() < 0.1
    assert r["accuracy"] == LR.CLS_ACCURACY and r["accuracy"] not in (0.0, 0.5, 1.0)
    # p - y is exactly 0 in float32 on some rows of the train forward: a positive above 16.7, a negative below -88.8
    l32 = r["train"].astype(np.float32)
    with np.errstate(over="ignore"):
        p = np.float32(1.0) / (np.float32(1.0) + np.exp(-l32))
    assert ((p - y) == 0.0).sum() >= 2 and ((p == 0.0) & (y == 0)).any() and ((p == 1.0) & (y == 1)).any()
    sc = reg["params"]["head/ln/scale"]
    assert (sc < 0).sum() >= 20 and (sc > 0).sum() >= 20
    # the naive softplus log(1 + exp(x)) is NOT as good here: it overflows on a row
    with np.errstate(over="ignore"):
        assert np.isinf(np.log1p(np.exp(np.abs(l32)))).any()


# ---- attainability: what plain float32 reaches under the measures of the GPU tests ----------------------------------------------------
@pytest.mark.parametrize("which", LR.BC_SETS)
def test_plain_fp32_attains_the_bound_in_the_bc_regime(which):
    cfg, B = LR.BC_CFG, LR.BC_B
    r64, r32 = LR.bc_run(cfg, B, which), LR.bc_run(cfg, B, which, torch.float32)
    wi = max(abs(r32["info"][k] - v) / max(1.0, abs(v)) for k, v in r64["info"].items())
    wg = max(LR.rel_err(r32["grads"][k], r64["grads"][k]) for k in BO.TRAIN)
    wc = max(float(np.nanmax(LR.column_errors(cfg.A, r32["grads"][k], r64["grads"][k]))) for k in BO.HEAD_LEAVES)
    print(f"bc {which}: float32 oracle vs fp64: infos {wi:.1e}, gradient leaves {wg:.1e}, head columns {wc:.1e}")
    assert wi <= F32_YARDSTICK and wg <= F32_YARDSTICK and wc <= F32_YARDSTICK, (wi, wg, wc)


def test_plain_fp32_attains_the_bound_in_the_classifier_regime():
    """the oracle in float32 throughout, the frozen trunk included"""
    r64, r32 = LR.cls_run(), LR.cls_run(torch.float32)
    wi = abs(r32["loss"] - r64["loss"]) / abs(r64["loss"])
    wl = max(np.abs(r32[k] - r64[k]).max() / np.abs(r64[k]).max() for k in ("eval", "train"))
    wg = max(LR.rel_err(r32["grads"][k], g) for k, g in r64["grads"].items())
    print(f"classifier regime: float32 oracle vs fp64: loss {wi:.1e}, logits {wl:.1e}, gradient leaves {wg:.1e}, accuracy {r32['accuracy']}")
    assert r32["accuracy"] == r64["accuracy"]
    assert wi <= F32_YARDSTICK and wl <= F32_YARDSTICK and wg <= F32_YARDSTICK, (wi, wl, wg)


# ---- the edge tables -------------------------------------------------------------------------------------------------------------------
def test_the_edge_tables_hold_every_class():
    bs = [r[2] for r in LR.BC_EDGES]
    assert {1, 7, 255, 257, 520} <= set(bs)
    assert any(b < LR.BC_TRIP for b in bs) and LR.BC_TRIP + 1 in bs and any(b > 2 * LR.BC_TRIP for b in bs)   # < one trip, one trip + 1, > two
    assert {1, 33, 64} <= {r[3] for r in LR.BC_EDGES} and LR.BC_A_REFUSED == 65
    assert {1, 65, 130} <= {r[4] for r in LR.BC_EDGES}
    assert {1, 3, LR.MAX_CAMS} <= {r[1] for r in LR.BC_EDGES}
    with open(os.path.join(HERE, "..", "include", "serl_mi355.h")) as f:
        assert f"#define SERL_MAX_CAMS {LR.MAX_CAMS}" in " ".join(f.read().split())
    for row in LR.BC_EDGES:
        cfg, B = LR.bc_edge_cfg(row)
        assert (cfg.H, cfg.W) == (32, 32) and cfg.n_cam == row[1]
    cb = [r[2] for r in LR.CLS_EDGES]
    assert {1, 2, 5, 7, 257, 300} <= set(cb)
    assert {1, 2, 3} <= {b % LR.CLS_ROWS_PER_WG for b in cb} and any(b > LR.CLS_INFO_TRIP for b in cb)
    assert {1, 3, LR.MAX_CAMS} <= {r[1] for r in LR.CLS_EDGES}
    keys, _, frames, labels, _ = LR.cls_edge(LR.CLS_EDGES[0])
    assert labels.shape == (1,) and frames[keys[0]].shape == (1, 1, 32, 32, 3)
    assert set(LR.cls_edge(LR.CLS_EDGES[3])[3]) == {0.0, 1.0}
