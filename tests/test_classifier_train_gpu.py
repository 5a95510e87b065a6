"""GPU: reward-classifier training in libserl_mi355.so (csrc/classifier.hip) through serl_amd.networks.reward_classifier
against the reference's own training loop (tests/golden/classifier_train_*.npz, see test_classifier_train_cpu.py) and the
fp64 restatement (tests/classifier_train_oracle.py): per-step loss / accuracy, final params and Adam moments, frozen trunk,
drawn vs injected Dropout masks, the device crop, the timed shape (B = 256, 2 x 128x128), checkpoints, the loop on HBM
data stores, and the error paths."""
import ctypes as C
import itertools
import json
import os
import pickle

import numpy as np
import pytest
import torch

import classifier_train_oracle as CT
from oracle import classifier_oracle as CO
from oracle import golden_update as G
from test_classifier_train_cpu import CASES, epoch_frames, golden_masks, load_case

pytestmark = pytest.mark.gpu


def _classifier(keys, H, W, params, max_batch, lr=1e-4):
    from serl_amd.networks.reward_classifier import Classifier
    return Classifier(keys, H, W, max_batch=max_batch, trainable=True, learning_rate=lr).load_flat(params)


def _golden_batches(d, meta, keys):
    from serl_amd import jaxrng as J
    B, H, W = meta["B"], meta["H"], meta["W"]
    data_rng = np.random.default_rng(meta["data_seed"])
    labels = np.concatenate([np.ones((B // 2, 1)), np.zeros((B // 2, 1))]).astype(np.float32)
    for e in range(meta["epochs"]):
        frames = epoch_frames(data_rng, keys, B, H, W)
        off = J.crop_offsets(d[f"e{e}_crop_key"], B, padding=4)
        data = {k: CT.host_crop(v[:, 0], off)[:, None] for k, v in frames.items()}
        yield e, {"data": data, "labels": labels}


def _run_golden(name, drawn):
    from serl_amd.networks.reward_classifier import train_step
    d, meta, keys = load_case(name)
    params = CO.make_params(keys, meta["H"], meta["W"], meta["param_seed"])
    c = _classifier(keys, meta["H"], meta["W"], params, meta["B"])
    out = []
    for e, batch in _golden_batches(d, meta, keys):
        masks = None if drawn else {k: m.astype(np.uint8) for k, m in golden_masks(d, e, keys, meta["B"]).items()}
        c, loss, acc = train_step(c, batch, d[f"e{e}_key"], masks=masks)
        out.append((float(loss), float(acc)))
    return d, meta, keys, params, c, out


@pytest.mark.parametrize("name", CASES)
def test_train_loop_equals_the_reference(gpu, name):
    d, meta, keys, params, c, out = _run_golden(name, drawn=False)
    lr, steps = meta["lr"], meta["epochs"]
    for e, (loss, acc) in enumerate(out):
        ref = float(d[f"e{e}_loss"])
        print(f"{name} epoch {e}: loss {loss:.6f} (reference {ref:.6f}), accuracy {acc} ({float(d[f'e{e}_accuracy'])})")
        assert abs(loss - ref) < 1e-4 * abs(ref)
        assert np.float32(acc) == np.float32(d[f"e{e}_accuracy"])   # (a float32 mean of the same hits)
    assert c.step == meta["final_step"]
    for leaf in CT.trainable(keys):
        got = c.get(c._leaf(leaf.split("/")[1], leaf.split("/", 2)[2]) if leaf.startswith("enc/") else leaf)
        rec = {kind: d[f"f_params|{leaf}|{kind}"] for kind in ("full", "stat", "val") if f"f_params|{leaf}|{kind}" in d.files}
        ref = rec["full"] if "full" in rec else rec["val"]
        g = got.astype(np.float64) if "full" in rec else got.astype(np.float64)[G._sample_idx(got.size, G._salt(f"params/{leaf}"))]
        diff = np.abs(g - ref)
        assert np.percentile(diff, 99.9) < 1e-4 and diff.max() <= 2 * lr * steps, (leaf, np.percentile(diff, 99.9), diff.max())
        for sec in ("mu", "nu"):
            m = c._get(f"opt/{sec}", c._leaf(leaf.split("/")[1], leaf.split("/", 2)[2]) if leaf.startswith("enc/") else leaf)
            rec = {kind: d[f"f_{sec}|{leaf}|{kind}"] for kind in ("full", "stat", "val") if f"f_{sec}|{leaf}|{kind}" in d.files}
            ref = rec["full"] if "full" in rec else rec["val"]
            mm = m.astype(np.float64) if "full" in rec else m.astype(np.float64)[G._sample_idx(m.size, G._salt(f"{sec}/{leaf}"))]
            assert np.abs(mm - ref).max() <= 1e-4 * np.abs(ref).max() + 1e-30, (sec, leaf)
    # the frozen trunk: bit-identical, zero moments
    for leaf in (k for k in params if k.startswith("trunk/")):
        assert np.array_equal(c.get(leaf), params[leaf].reshape(-1)), leaf
        assert not np.any(c._get("opt/mu", leaf)) and not np.any(c._get("opt/nu", leaf))


@pytest.mark.parametrize("name", CASES)
def test_drawn_masks_equal_injected_masks_bit_for_bit(gpu, name):
    *_, a, out_a = _run_golden(name, drawn=False)
    *_, b, out_b = _run_golden(name, drawn=True)
    assert out_a == out_b
    for leaf in a._counts:
        assert np.array_equal(a.get(leaf), b.get(leaf)), leaf
        if not leaf.startswith("trunk/"):
            assert np.array_equal(a._get("opt/nu", leaf), b._get("opt/nu", leaf)), leaf


def test_train_mode_logits_and_the_inference_handle(gpu):
    from serl_amd import _lib
    from serl_amd.networks.reward_classifier import Classifier
    d, meta, keys = load_case("one_cam_64")
    params = CO.make_params(keys, meta["H"], meta["W"], meta["param_seed"])
    c = _classifier(keys, meta["H"], meta["W"], params, meta["B"])
    e, batch = next(_golden_batches(d, meta, keys))
    masks = golden_masks(d, 0, keys, meta["B"])
    feats = CT.features(params, keys, {k: v[:, 0] for k, v in batch["data"].items()})
    th = {k: torch.tensor(np.asarray(v), dtype=torch.float64) for k, v in params.items()}
    ref = CT.forward(th, keys, feats, masks).numpy()
    got = c.apply_fn({"params": c.params}, batch["data"], train=True, rngs={"dropout": d["e0_key"]})
    assert got.shape == (meta["B"], 1) and np.abs(got - ref).max() < 1e-4
    assert np.abs(c.apply_fn({"params": c.params}, batch["data"]) - CT.forward(th, keys, feats).numpy()).max() < 1e-4
    assert c.step == 0   # apply_fn does not update
    # an inference-only handle has no training state
    inf = Classifier(keys, meta["H"], meta["W"], max_batch=meta["B"]).load_flat(params)
    with pytest.raises(NotImplementedError):
        inf.apply_fn({"params": inf.params}, batch["data"], train=True, rngs={"dropout": d["e0_key"]})
    with pytest.raises(NotImplementedError):
        inf.train_step(batch, d["e0_key"])
    fr = torch.zeros((1, 2, meta["H"], meta["W"], 3), dtype=torch.uint8, device="cuda")
    lab = torch.zeros(2, device="cuda")
    keys_host = np.zeros(4, np.uint32)
    rc = inf.L.serl_classifier_train_step(inf._h, C.c_void_p(fr.data_ptr()), 2, C.c_void_p(lab.data_ptr()), None,
                                          keys_host.ctypes.data_as(C.c_void_p), None)
    assert rc == -3   # SERL_ERR_STATE
    out = C.c_int64()
    assert inf.L.serl_classifier_train_get_step(inf._h, C.byref(out)) == -3
    # n > max_batch
    big = {k: np.concatenate([v, v]) for k, v in batch["data"].items()}
    with pytest.raises(_lib.SerlError):
        c.train_step({"data": big, "labels": np.zeros((2 * meta["B"], 1), np.float32)}, d["e0_key"])
    assert c.step == 0


def test_one_step_at_the_timed_shape_equals_the_fp64_restatement(gpu):
    from serl_amd.networks.reward_classifier import train_step
    keys, H, W, B = ("front", "wrist"), 128, 128, 256
    params = CO.make_params(keys, H, W, 31)
    rng = np.random.default_rng(32)
    frames = {k: rng.integers(0, 256, (B, 1, H, W, 3), dtype=np.uint8) for k in keys}
    masks = {k: rng.random((B, 4096)) < 0.9 for k in keys}
    masks["head"] = rng.random((B, 256)) < 0.9
    labels = np.concatenate([np.ones((B // 2, 1)), np.zeros((B // 2, 1))]).astype(np.float32)
    st = CT.State(params, keys)
    feats = CT.features(params, keys, {k: v[:, 0] for k, v in frames.items()})
    loss_ref, acc_ref, ev, grads = CT.train_step(st, feats, labels, masks)
    c = _classifier(keys, H, W, params, B)
    c, loss, acc = train_step(c, {"data": frames, "labels": labels}, None, masks={k: m.astype(np.uint8) for k, m in masks.items()})
    loss, acc = float(loss), float(acc)
    print(f"B=256 2x128x128: loss {loss:.6f} (fp64 {loss_ref:.6f}), accuracy {acc} ({acc_ref}), min |eval logit| {np.abs(ev).min():.2e}")
    assert abs(loss - loss_ref) < 1e-4 * abs(loss_ref)
    assert np.float32(acc) == np.float32(acc_ref)
    for leaf, g in grads.items():   # the step-1 moments are the gradient: mu = 0.1 g, nu = 0.001 g^2
        name = f"enc/{keys.index(leaf.split('/')[1])}/{leaf.split('/', 2)[2]}" if leaf.startswith("enc/") else leaf
        mu, nu = c._get("opt/mu", name).astype(np.float64), c._get("opt/nu", name).astype(np.float64)
        assert np.abs(mu - 0.1 * g).max() <= 1e-4 * np.abs(0.1 * g).max() + 1e-30, leaf
        assert np.abs(nu - 0.001 * g * g).max() <= 1e-4 * np.abs(0.001 * g * g).max() + 1e-30, leaf


def test_checkpoint_resume_and_load_classifier_func(gpu, tmp_path):
    from serl_amd.networks.reward_classifier import Classifier, load_classifier_func, train_step
    from serl_amd.utils.checkpoint import read_checkpoint_tree, restore_checkpoint, save_checkpoint
    d, meta, keys = load_case("one_cam_64")
    H, W, B = meta["H"], meta["W"], meta["B"]
    params = CO.make_params(keys, H, W, meta["param_seed"])
    batches = list(_golden_batches(d, meta, keys))
    K = 2

    def run(c, steps):
        for e in steps:
            c, _, _ = train_step(c, batches[e % len(batches)][1], d[f"e{e % len(batches)}_key"])
        return c

    full = run(_classifier(keys, H, W, params, B), range(2 * K))
    a = run(_classifier(keys, H, W, params, B), range(K))
    save_checkpoint(str(tmp_path / "ckpt"), a, step=K, overwrite=True)
    tree = read_checkpoint_tree(str(tmp_path / "ckpt"))
    assert sorted(tree) == ["opt_state", "params", "step"] and int(tree["step"]) == K
    assert sorted(tree["opt_state"]) == ["0", "1"] and sorted(tree["opt_state"]["0"]) == ["count", "mu", "nu"]
    # load_classifier_func reads it unchanged: the same logits as the trained handle
    pkl = tmp_path / "resnet10_params.pkl"
    from test_classifier_gpu import _pickle_tree
    with open(pkl, "wb") as f:
        pickle.dump(_pickle_tree(params), f)
    obs = batches[0][1]["data"]
    func = load_classifier_func(np.array([0, 1], np.uint32), obs, list(keys), str(tmp_path / "ckpt"), pretrained_encoder_path=str(pkl))
    assert np.array_equal(func(obs), a.logits(obs))
    # restore into a fresh trainable classifier and go on: bit-identical to the run without a break
    b = Classifier(keys, H, W, max_batch=B, trainable=True)
    restore_checkpoint(str(tmp_path / "ckpt"), b)
    assert b.step == K
    b = run(b, range(K, 2 * K))
    assert b.step == full.step == 2 * K
    for leaf in full._counts:
        assert np.array_equal(full.get(leaf), b.get(leaf)), leaf
        assert np.array_equal(full._get("opt/mu", leaf), b._get("opt/mu", leaf)), leaf


class _Sp:
    def __init__(self, shape):
        self.shape = shape


class _Obs:
    def __init__(self, keys, H, W, S):
        self.spaces = {k: _Sp((1, H, W, 3)) for k in keys}
        self.spaces["state"] = _Sp((1, S))


def _stores(keys, H, W, n, seed):
    from serl_amd.data.data_store import MemoryEfficientReplayBufferDataStore
    from serl_amd.utils.synthetic import transition_stream
    out = []
    for j in range(2):
        s = MemoryEfficientReplayBufferDataStore(_Obs(keys, H, W, 4), _Sp((2,)), n + 4, image_keys=list(keys))
        for t in itertools.islice(transition_stream(keys, H, W, 3, 1, 4, 2, 10, seed + j), n):
            s.insert(t)
        s.seed(seed + 10 + j)
        out.append(s)
    return out


def test_device_crop_equals_the_host_crop(gpu):
    from serl_amd import jaxrng as J
    from serl_amd.agents.batch import DeviceBatch
    from serl_amd.data.data_store import gather_crop
    keys, H, W, B = ("front", "wrist"), 64, 64, 6
    pos, _ = _stores(keys, H, W, 12, 5)
    idx = pos.sample_indices(B)
    off = J.crop_offsets(J.prngkey(3), B, padding=4)
    db = DeviceBatch(B, len(keys), H, W, 3, 4, 2, 0)
    gather_crop([(pos, idx.copy())], off, off, db)
    host = pos.gather(idx)
    for i, k in enumerate(keys):
        packed = host["observations"][k].cpu().numpy()   # [B, 2, H, W, 3]
        for side in (0, 1):
            assert np.array_equal(db.frames[side, i].cpu().numpy(), CT.host_crop(packed[:, side], off)), (k, side)


def test_train_reward_classifier_on_data_stores(gpu, tmp_path):
    from serl_amd import jaxrng as J
    from serl_amd.networks.reward_classifier import train_reward_classifier
    from serl_amd.utils.checkpoint import read_checkpoint_tree
    keys, H, W, B, E = ("front", "wrist"), 64, 64, 8, 3
    params = CO.make_params(keys, H, W, 41)
    pos, neg = _stores(keys, H, W, 20, 11)
    pkl = tmp_path / "resnet10_params.pkl"
    from test_classifier_gpu import _pickle_tree
    with open(pkl, "wb") as f:
        pickle.dump(_pickle_tree(params), f)
    c, log = train_reward_classifier(pos, neg, list(keys), batch_size=B, num_epochs=E, classifier_ckpt_path=str(tmp_path / "ck"),
                                     pretrained_encoder_path=str(pkl), init_params=params, verbose=False)
    # the same draws from stores seeded alike: one shape-only draw each, then B/2 per epoch
    p2, n2 = _stores(keys, H, W, 20, 11)
    p2.sample_indices(B // 2), n2.sample_indices(B // 2)
    rng = J.split(J.split(J.prngkey(0))[0])[0]
    st = CT.State(params, keys)
    labels = np.concatenate([np.ones(B // 2), np.zeros(B // 2)])
    for e in range(E):
        ip, ineg = p2.sample_indices(B // 2), n2.sample_indices(B // 2)
        assert np.array_equal(ip, log["pos_idx"][e]) and np.array_equal(ineg, log["neg_idx"][e])
        rng, ck = J.split(rng)
        off = J.crop_offsets(ck, B, padding=4)
        assert np.array_equal(off, log["crop"][e])
        rng, key = J.split(rng)
        gp, gn = p2.gather(ip), n2.gather(ineg)
        frames = {k: np.concatenate([gp["observations"][k].cpu().numpy()[:, 1], gn["observations"][k].cpu().numpy()[:, 0]]) for k in keys}
        from serl_amd.networks.reward_classifier import dropout_keys
        from test_classifier_train_cpu import bernoulli_host
        dk = dropout_keys(key, keys)
        masks = {k: bernoulli_host(dk[i], (B, 4096)) for i, k in enumerate(keys)}
        masks["head"] = bernoulli_host(dk[-1], (B, 256))
        feats = CT.features(params, keys, {k: CT.host_crop(v, off) for k, v in frames.items()})
        loss, acc, _, _ = CT.train_step(st, feats, labels, masks)
        assert abs(log["loss"][e] - loss) < 1e-4 * abs(loss) and np.float32(log["accuracy"][e]) == np.float32(acc), (e, log["loss"][e], loss)
    for leaf in CT.trainable(keys):
        name = f"enc/{keys.index(leaf.split('/')[1])}/{leaf.split('/', 2)[2]}" if leaf.startswith("enc/") else leaf
        diff = np.abs(c.get(name) - st.params[leaf])
        assert np.percentile(diff, 99.9) < 1e-4 and diff.max() <= 2 * 1e-4 * E, leaf
    assert int(read_checkpoint_tree(str(tmp_path / "ck"))["step"]) == E
