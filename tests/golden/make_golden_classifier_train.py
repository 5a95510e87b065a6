"""Generates tests/golden/classifier_train_*.npz: the reward-classifier training loop of the reference
(examples/async_cable_route_drq/train_reward_classifier.py:101-160) run on the reference's OWN BinaryClassifier /
create_classifier (serl_launcher/networks/reward_classifier.py) and batched_random_crop (vision/data_augmentations.py),
executed unmodified under the stand-ins of oracle/jaxshim in fp64 with jax.random's threefry (SERL_JAXSHIM_PRNG=threefry).
Run in the build container (needs the reference tree):
    python tests/golden/make_golden_classifier_train.py

The script's train_step (:122-137) is a closure inside its train_reward_classifier, so its ten lines are restated below
around the reference modules; optax.sigmoid_binary_cross_entropy, which the stand-in optax lacks, is restated from optax's
published definition (-labels * log_sigmoid(logits) - (1 - labels) * log_sigmoid(-logits)).  The script's data stores are
replaced by seeded frames (the store draws are the data stores' business, tested elsewhere).  The classifier's parameters
are overwritten with oracle.classifier_oracle.make_params (numpy-seeded: the tests rebuild them from the seed).

Recorded per epoch: the keys of the chain (crop and train step), the Dropout keep-masks the run drew (packed bits, with their
scope paths), loss and train_accuracy, and the eval logits; at the end the trainable params and Adam moments
(golden_update.leaf_record), the TrainState tree paths / shapes and the optimizer-state form, and the first two cropped
frames of camera 0 in epoch 0.

A case may carry two hooks: a frame builder (keys, H, W, B, epochs) -> [frames of epoch e] in place of the seeded noise, and a
parameter transform (keys, H, W, param seed, [cropped frames of epoch e]) -> params in place of make_params alone.
regime_one_cam_64 uses them to run the loop in the regime of tests/learner_regimes.py: structured frames and a hand-built head whose
logits span both signs from below 1 to beyond 90.
"""
import json
import os
import pickle
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["SERL_JAXSHIM_PRNG"] = "threefry"
from oracle import ref_update_shim as R   # noqa: E402

R.install(True)
import jax   # noqa: E402
import jax.numpy as jnp   # noqa: E402
from flax.core.frozen_dict import freeze   # noqa: E402
from oracle import classifier_oracle as CO, golden_update as G, ref_update_runner as RR   # noqa: E402
from serl_amd.networks.reward_classifier import _CAM_PATHS, _HEAD_PATHS   # noqa: E402  (pure-python path tables)
from serl_launcher.networks.reward_classifier import create_classifier   # noqa: E402
from serl_launcher.vision.data_augmentations import batched_random_crop   # noqa: E402

# name: (image keys, H, W, batch, epochs, param seed, data seed)
CASES = {"two_cams_128": (("front", "wrist"), 128, 128, 8, 3, 21, 500),
         "one_cam_64": (("image",), 64, 64, 6, 3, 22, 600),
         # the regime of tests/learner_regimes.py (CLS_GOLDEN, CLS_KEYS, CLS_H, CLS_W, CLS_GOLDEN_B, CLS_PARAM_SEED); no data seed: its frames are built
         "regime_one_cam_64": (("image",), 64, 64, 6, 2, 23, 0)}


def hooks(name, case):
    """-> (frame builder, parameter transform, what meta["regime"] says of them) of a case; built only for the case that has them"""
    if name != "regime_one_cam_64":
        return None, None, None
    import learner_regimes as LR
    assert name == LR.CLS_GOLDEN and case[:4] == (LR.CLS_KEYS, LR.CLS_H, LR.CLS_W, LR.CLS_GOLDEN_B) and case[5] == LR.CLS_PARAM_SEED
    return (LR.cls_golden_frames, LR.cls_golden_params,
            {"frames": "cls_golden_frames", "params": "cls_golden_params", "targets": list(LR.CLS_GOLDEN_TARGETS)})


def sigmoid_binary_cross_entropy(logits, labels):
    """optax/_src/loss.py sigmoid_binary_cross_entropy (restated: the stand-in optax has no losses)"""
    log_p = -jax.nn.softplus(-logits)
    log_not_p = -jax.nn.softplus(logits)
    return -labels * log_p - (1.0 - labels) * log_not_p


def put(tree, path, v):
    d = tree
    for p in path[:-1]:
        d = d[p]
    assert tuple(d[path[-1]].shape) == tuple(np.shape(v)), (path, d[path[-1]].shape, np.shape(v))
    d[path[-1]] = jnp.asarray(np.asarray(v, np.float64))


def flat(tree, pre=()):
    if hasattr(tree, "items"):
        for k, v in tree.items():
            yield from flat(v, pre + (k,))
    else:
        yield pre, tree


def ints(key):
    return np.array([int(v) & 0xFFFFFFFF for v in np.asarray(key).reshape(-1)], np.uint32)


def epoch_frames(data_rng, keys, B, H, W):
    """The frames of one epoch (the tests regenerate them from the data seed: epochs draw in order, cameras in key order)"""
    return {k: data_rng.integers(0, 256, (B, 1, H, W, 3), dtype=np.uint8) for k in keys}


def leaf_paths(keys):
    out = {}
    for k in keys:
        for leaf, sub in _CAM_PATHS.items():
            out[f"enc/{k}/{leaf}"] = ("encoder_def", f"encoder_{k}") + sub
    for leaf, sub in _HEAD_PATHS.items():
        out[leaf] = sub
    return out


def run_case(keys, H, W, B, epochs, pseed, dseed, frames_fn=None, params_fn=None, regime=None):
    params0 = CO.make_params(keys, H, W, pseed)
    d = tempfile.mkdtemp()
    pkl = os.path.join(d, "resnet10_params.pkl")
    with open(pkl, "wb") as f:
        pickle.dump(RR.pretrained_pickle_tree({k: v for k, v in params0.items() if k.startswith("trunk/")}), f)
    rec = {}
    # train_reward_classifier.py:101-108
    rng = jax.random.PRNGKey(0)
    rng, key = jax.random.split(rng)
    rng, key = jax.random.split(rng)
    sample = {k: jnp.asarray(np.zeros((B, 1, H, W, 3), np.uint8)) for k in keys}
    classifier = create_classifier(key, sample, list(keys), pretrained_encoder_path=pkl)
    tree = classifier.params.unfreeze()
    hw = (H // 32) * (W // 32)
    side = int(round(hw ** 0.5))
    paths = leaf_paths(keys)
    data_rng = np.random.default_rng(dseed)
    all_frames = frames_fn(keys, H, W, B, epochs) if frames_fn else [epoch_frames(data_rng, keys, B, H, W) for _ in range(epochs)]
    if params_fn is not None:   # the crops the loop below will draw: the same key chain, walked ahead on a copy
        r, cropped = rng, []
        for e in range(epochs):
            r, ck = jax.random.split(r)
            r, _ = jax.random.split(r)
            cropped.append({k: np.asarray(batched_random_crop(jnp.asarray(v), ck, padding=4, num_batch_dims=2)).astype(np.uint8)[:, 0]
                            for k, v in all_frames[e].items()})
        params0 = params_fn(keys, H, W, pseed, cropped)
    for name, path in paths.items():
        v = params0[name]
        if name.endswith("/sle"):
            v = v.reshape(side, hw // side, 512, 8)
        put(tree, path, np.asarray(v).reshape(tuple(np.shape(_get(tree, path)))))
    classifier = classifier.replace(params=freeze(tree))
    rec["tree_paths"] = np.array(["/".join(p) for p, _ in flat(classifier.params)])
    rec["tree_shapes"] = np.array([json.dumps(list(np.shape(v))) for _, v in flat(classifier.params)])
    opt_form = [{"type": type(s).__name__, "fields": list(getattr(s, "_fields", None) or [])} for s in classifier.opt_state]
    trunk0 = {"/".join(p): np.asarray(v, np.float64).copy() for p, v in flat(classifier.params) if "pretrained_encoder" in p}

    @jax.jit
    def train_step(state, batch, key):   # train_reward_classifier.py:122-137
        def loss_fn(params):
            logits = state.apply_fn({"params": params}, batch["data"], rngs={"dropout": key}, train=True)
            return sigmoid_binary_cross_entropy(logits, batch["labels"]).mean()

        grad_fn = jax.value_and_grad(loss_fn)
        loss, grads = grad_fn(state.params)
        logits = state.apply_fn({"params": state.params}, batch["data"], train=False, rngs={"dropout": key})
        train_accuracy = jnp.mean((jax.nn.sigmoid(logits) >= 0.5) == batch["labels"])
        return state.apply_gradients(grads=grads), loss, train_accuracy, logits

    rec["rng0"] = ints(rng)
    for e in range(epochs):
        frames = all_frames[e]   # [pos next_observations; neg observations]
        rng, key = jax.random.split(rng)
        rec[f"e{e}_crop_key"] = ints(key)
        cropped = {k: batched_random_crop(jnp.asarray(v), key, padding=4, num_batch_dims=2) for k, v in frames.items()}
        labels = jnp.concatenate([jnp.ones((B // 2, 1)), jnp.zeros((B // 2, 1))], axis=0)
        batch = {"data": freeze(cropped), "labels": labels}
        rng, key = jax.random.split(rng)
        rec[f"e{e}_key"] = ints(key)
        tape = jax.random.start_tape()
        classifier, loss, acc, logits = train_step(classifier, batch, key)
        jax.random.stop_tape()
        drawn = [r for r in tape if r["kind"] == "bernoulli"]
        ctx = [r["context"][-1] for r in drawn]
        rec[f"e{e}_mask_paths"] = np.array(ctx)
        for r in drawn:
            tag = r["context"][-1].split(":", 1)[1]
            rec[f"e{e}_mask|{tag}"] = np.packbits(np.asarray(r["value"]).astype(np.uint8), axis=None)
            rec[f"e{e}_mask_shape|{tag}"] = np.array(np.shape(r["value"]))
        rec[f"e{e}_loss"] = np.float64(np.asarray(loss))
        rec[f"e{e}_accuracy"] = np.float64(np.asarray(acc))
        rec[f"e{e}_logits_eval"] = np.asarray(logits, np.float64)
        # the crop: every camera, sample i shifted by the same offset (one key) -- recorded from the result itself
        if e == 0:
            rec["e0_cropped_" + keys[0]] = np.asarray(cropped[keys[0]]).astype(np.uint8)[:2]
    st = classifier
    adam = st.opt_state[0]
    for name, path in paths.items():
        for sec, t in (("params", st.params), ("mu", adam.mu), ("nu", adam.nu)):
            for kind, arr in G.leaf_record(f"{sec}/{name}", np.asarray(_get(t, path), np.float64)).items():
                rec[f"f_{sec}|{name}|{kind}"] = arr
    for p, v in flat(st.params):
        key = "/".join(p)
        if key in trunk0:
            assert np.array_equal(np.asarray(v, np.float64), trunk0[key]), key
    for t in (adam.mu, adam.nu):
        for p, v in flat(t):
            if "pretrained_encoder" in p:
                assert not np.any(np.asarray(v)), p
    meta = {"image_keys": list(keys), "H": H, "W": W, "B": B, "epochs": epochs, "param_seed": pseed, "data_seed": dseed,
            "final_step": int(np.asarray(st.step)), "opt_state": opt_form, "lr": 1e-4}
    if regime is not None:
        meta["regime"] = regime
    rec["meta"] = np.array(json.dumps(meta))
    return rec


def _get(tree, path):
    for p in path:
        tree = tree[p]
    return tree


def main():
    out_dir = os.path.dirname(os.path.abspath(__file__))
    only = [a for a in sys.argv[1:] if not a.startswith("-")]
    for name, case in CASES.items():
        if only and name not in only:
            continue
        rec = run_case(*case, *hooks(name, case))
        path = os.path.join(out_dir, f"classifier_train_{name}.npz")
        np.savez_compressed(path, **rec)
        meta = json.loads(str(rec["meta"]))
        print(name, "->", path, f"{os.path.getsize(path) / 1e6:.2f} MB",
              [float(rec[f"e{e}_loss"]) for e in range(meta["epochs"])], [float(rec[f"e{e}_accuracy"]) for e in range(meta["epochs"])])


if __name__ == "__main__":
    main()
