"""CPU: reward-classifier training against tests/golden/classifier_train_*.npz, written by
tests/golden/make_golden_classifier_train.py from the reference's own BinaryClassifier / create_classifier /
batched_random_crop under oracle/jaxshim (fp64, jax.random's threefry):
  - the Dropout layers' scope paths and the loop's key chain (crop keys, train-step keys, per-layer make_rng keys ->
    keep-masks, crop offsets -> cropped frames) are bit-exact with the library's host functions only;
  - the fp64 restatement of the train step (tests/classifier_train_oracle.py) reproduces the golden losses, accuracies, eval
    logits, final params and Adam moments;
  - the trainable classifier's state tree (paths, shapes, optax.adam's state form) is the reference's TrainState tree."""
import json
import os

import numpy as np
import pytest

import classifier_train_oracle as CT
from oracle import classifier_oracle as CO
from oracle import golden_update as G

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["two_cams_128", "one_cam_64"]


def load_case(name):
    d = np.load(os.path.join(HERE, "golden", f"classifier_train_{name}.npz"))
    meta = json.loads(str(d["meta"]))
    return d, meta, tuple(meta["image_keys"])


def epoch_frames(data_rng, keys, B, H, W):
    """(as the generator draws them)"""
    return {k: data_rng.integers(0, 256, (B, 1, H, W, 3), dtype=np.uint8) for k in keys}


def golden_masks(d, e, keys, B):
    from serl_amd.networks.reward_classifier import dropout_paths
    out = {}
    for k, path in zip(list(keys) + ["head"], dropout_paths(keys)):
        tag = "/".join(path)
        shape = tuple(int(v) for v in d[f"e{e}_mask_shape|{tag}"])
        out[k] = np.unpackbits(d[f"e{e}_mask|{tag}"])[:int(np.prod(shape))].reshape(shape).astype(bool)
    return out


def bernoulli_host(key, shape, p=0.9):
    """jax.random.bernoulli(key, p, shape) from the library's host threefry: uniform(bits) < p in float32"""
    from serl_amd import jaxrng as J
    bits = J.random_bits(key, int(np.prod(shape)))
    u = ((bits >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1.0)
    return (u < np.float32(p)).reshape(shape)


@pytest.mark.parametrize("name", CASES)
def test_dropout_paths_and_key_chain_are_bit_exact(name):
    from serl_amd import jaxrng as J
    from serl_amd.networks.reward_classifier import dropout_keys, dropout_paths
    d, meta, keys = load_case(name)
    B, H, W = meta["B"], meta["H"], meta["W"]
    for e in range(meta["epochs"]):
        assert [str(p) for p in d[f"e{e}_mask_paths"]] == ["dropout:" + "/".join(p) for p in dropout_paths(keys)]
    # train_reward_classifier.py:101-107 then two splits per epoch (:148, :159)
    rng = J.prngkey(0)
    rng, _ = J.split(rng)
    rng, _ = J.split(rng)
    assert np.array_equal(rng, d["rng0"])
    data_rng = np.random.default_rng(meta["data_seed"])
    for e in range(meta["epochs"]):
        frames = epoch_frames(data_rng, keys, B, H, W)
        rng, crop_key = J.split(rng)
        assert np.array_equal(crop_key, d[f"e{e}_crop_key"])
        rng, key = J.split(rng)
        assert np.array_equal(key, d[f"e{e}_key"])
        masks = golden_masks(d, e, keys, B)
        for (k, m), dk in zip(masks.items(), dropout_keys(key, keys)):
            assert np.array_equal(bernoulli_host(dk, m.shape), m), (e, k)
        if e == 0:   # one key for every camera: offsets of sample i from split(key, B)[i]
            off = J.crop_offsets(crop_key, B, padding=4)
            got = CT.host_crop(frames[keys[0]][:, 0], off)[:2]
            assert np.array_equal(got, d[f"e0_cropped_{keys[0]}"][:, 0])


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference_train_loop(name):
    from serl_amd import jaxrng as J
    d, meta, keys = load_case(name)
    B, H, W = meta["B"], meta["H"], meta["W"]
    params = CO.make_params(keys, H, W, meta["param_seed"])
    st = CT.State(params, keys, lr=meta["lr"])
    data_rng = np.random.default_rng(meta["data_seed"])
    labels = np.concatenate([np.ones(B // 2), np.zeros(B // 2)])
    for e in range(meta["epochs"]):
        frames = epoch_frames(data_rng, keys, B, H, W)
        off = J.crop_offsets(d[f"e{e}_crop_key"], B, padding=4)
        feats = CT.features(params, keys, {k: CT.host_crop(v[:, 0], off) for k, v in frames.items()})
        loss, acc, ev, _ = CT.train_step(st, feats, labels, golden_masks(d, e, keys, B))
        assert abs(loss - float(d[f"e{e}_loss"])) < 1e-9 * max(1.0, abs(loss)), (e, loss, float(d[f"e{e}_loss"]))
        assert acc == float(d[f"e{e}_accuracy"])
        assert np.abs(ev - d[f"e{e}_logits_eval"]).max() < 1e-9
    assert st.step == meta["final_step"]
    for name_ in CT.trainable(keys):
        for sec, v in (("params", st.params[name_]), ("mu", st.mu[name_]), ("nu", st.nu[name_])):
            rec = {kind: d[f"f_{sec}|{name_}|{kind}"] for kind in ("full", "stat", "val") if f"f_{sec}|{name_}|{kind}" in d.files}
            err, how = G.leaf_compare(f"{sec}/{name_}", rec, v)
            assert err < 1e-9, (sec, name_, err, how)


@pytest.mark.parametrize("name", CASES)
def test_state_tree_is_the_reference_train_state(name):
    from serl_amd.agents.flax_tree import _trunk_paths, trunk_owner
    from serl_amd.networks.reward_classifier import _CAM_PATHS, _HEAD_PATHS, EmptyState, ScaleByAdamState
    from serl_amd.utils.init import trunk_shapes
    d, meta, keys = load_case(name)
    H, W = meta["H"], meta["W"]
    side = H // 32
    want = {}
    for k in keys:
        for leaf, sub in _CAM_PATHS.items():
            shape = {"sle": [side, W // 32, 512, 8], "dense/kernel": [4096, 256]}.get(leaf, [256])
            want["/".join(("encoder_def", f"encoder_{k}") + sub)] = shape
    tsh = trunk_shapes()
    for leaf, sub in _trunk_paths().items():
        want["/".join(("encoder_def", f"encoder_{trunk_owner(keys)}", "pretrained_encoder") + tuple(sub))] = list(tsh[leaf])
    for leaf, sub in _HEAD_PATHS.items():
        want["/".join(sub)] = {"head/dense0/kernel": [256 * len(keys), 256], "head/dense1/kernel": [256, 1],
                               "head/dense1/bias": [1]}.get(leaf, [256])
    got = {str(p): json.loads(str(s)) for p, s in zip(d["tree_paths"], d["tree_shapes"])}
    assert got == want
    assert meta["opt_state"] == [{"type": "ScaleByAdamState", "fields": list(ScaleByAdamState._fields)},
                                 {"type": "EmptyState", "fields": list(EmptyState._fields)}]
