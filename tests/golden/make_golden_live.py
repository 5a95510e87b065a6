"""Generates the fixtures of the tests that compare the oracle against the reference's own code (tests/test_reference_update.py,
tests/test_replay_oracle.py, tests/test_host_logic.py): the reference is imported from its checkout (oracle/ref_shim.py,
oracle/ref_update_shim.py), run UNMODIFIED on exactly the inputs those tests use, and what it returned is stored here, so the
tests themselves need nothing outside the repository.  Run in the build container (needs the reference checkout):
    python tests/golden/make_golden_live.py
"""
import ast
import hashlib
import itertools
import json
import os
import pickle
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from oracle import golden_update as G  # noqa: E402
from oracle import drq_oracle as O  # noqa: E402
from oracle import ref_shim  # noqa: E402
from oracle import ref_update_runner as RR  # noqa: E402
from oracle import ref_update_shim as RS  # noqa: E402

# the reference runs of tests/test_reference_update.py: name -> (cfg, B, schedule, param_seed, batch_seed, prng)
UPDATE_CASES = {
    # the peg-insertion key names / dims, CAR-style schedule
    "peg": (O.Config(image_keys=("wrist_1", "wrist_2"), H=64, W=64, S=19, A=7), 4,
            [("critics",), ("high_utd", 2), ("critics",)], 7, 55, "philox"),
    # the stand-in jax.random drawing through JAX's own threefry2x32 key chain
    "key_chain": (O.Config(image_keys=("front",), H=64, W=64, S=7, A=4), 4, [("critics",), ("high_utd", 1)], 3, 11, "threefry"),
}


def _save(name, rec):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **rec)
    print(name, f"{os.path.getsize(path) / 1e6:.2f} MB")


# record form of the final train state (oracle/golden_update.py leaf_record): leaves of up to FULL_MAX elements whole, larger
# ones as N_SAMPLE fixed elements plus three whole-tensor projections; stored in each file so that the tests compare in kind
FULL_MAX, N_SAMPLE = 256, 256


def update_runs():
    for name, (cfg, B, sched, pseed, bseed, prng) in UPDATE_CASES.items():
        if prng == "threefry":
            os.environ["SERL_JAXSHIM_PRNG"] = "threefry"
        else:
            os.environ.pop("SERL_JAXSHIM_PRNG", None)
        res = RR.run_reference(cfg, B, sched, pseed, bseed)
        res["prng"] = os.environ.pop("SERL_JAXSHIM_PRNG", "philox")
        rec = G.pack(res, pseed, bseed, n_sample=N_SAMPLE, full_max=FULL_MAX)
        f = res["final"]
        rec["record_form"] = np.array([FULL_MAX, N_SAMPLE], np.int64)
        rec["count"] = np.array([f["count"][tx] for tx in O.TX_NAMES], np.int64)
        if "trunk_conv_init" in f:
            # the frozen trunk after the schedule: its exact bytes (fp64) and how far the target copy drifted from it
            rec["trunk_conv_init_sha256"] = np.array(hashlib.sha256(np.ascontiguousarray(f["trunk_conv_init"], np.float64).tobytes()).hexdigest())
            rec["trunk_conv_init_target_drift"] = np.float64(np.abs(f["trunk_conv_init_target"] - f["trunk_conv_init"]).max())
        # the final-state records (f_<section>|<leaf>|<kind>, a few hundred small arrays) as ONE fp64 array plus an index
        keys = sorted(k for k in rec if k.startswith("f_"))
        rec["final_index"] = np.array(json.dumps([[k, int(np.asarray(rec[k]).size)] for k in keys]))
        rec["final_data"] = np.concatenate([np.asarray(rec.pop(k), np.float64).reshape(-1) for k in keys])
        _save(f"live_update_{name}.npz", rec)


def param_tree():
    """agent.state.params of the reference (its own make_drq_agent + load_resnet10_params on a synthetic pickle): shapes only."""
    cfg = O.Config(image_keys=("front", "wrist"), H=64, W=64, S=5, A=3)
    res = RR.run_reference(cfg, 2, [], param_seed=1)
    def lists(t):          # leaves are shape tuples
        return {k: lists(v) for k, v in t.items()} if isinstance(t, dict) else list(t)

    tree = lists(res["final"]["param_tree"])
    path = os.path.join(HERE, "live_param_tree.json")
    with open(path, "w") as fh:
        json.dump(tree, fh, indent=1, sort_keys=True)
    print("live_param_tree.json")


def random_crop():
    """vision/data_augmentations.py:7-36 (edge pad 4 + dynamic_slice) on a seeded image batch: the crops and the offsets drawn."""
    jax = RS.install(True)
    import jax.numpy as jnp
    from serl_launcher.vision.data_augmentations import batched_random_crop
    img = np.random.default_rng(0).integers(0, 256, (6, 1, 24, 20, 3), dtype=np.uint8)
    tape = jax.random.start_tape()
    out = np.asarray(batched_random_crop(jnp.asarray(img), jax.random.PRNGKey(3), padding=4, num_batch_dims=2))
    jax.random.stop_tape()
    offs = np.stack([r["value"] for r in tape]).astype(np.int32)
    _save("live_random_crop.npz", {"out": out, "offs": offs})


def replay_buffers():
    from serl_amd.utils.synthetic import flat_stream, transition_stream
    # MemoryEfficientReplayBuffer (memory_efficient_replay_buffer.py): validity mask after every insert, packed samples
    keys, H, W, C, T, S, A, cap = ("a", "b"), 16, 16, 3, 1, 4, 2, 23
    Ref = ref_shim.load_reference_buffer_cls()
    osp, asp = ref_shim.make_spaces(keys, H, W, C, T, S, A)
    ref = Ref(osp, asp, cap, pixel_keys=keys)
    ref.seed(9)
    rec = {}
    for n, tr in enumerate(itertools.islice(transition_stream(keys, H, W, C, T, S, A, 5, 77), 120)):
        ref.insert(tr)
        rec[f"valid_{n}"] = np.asarray(ref._is_correct_index).copy()
        if n % 7 == 6:
            rb = ref.sample(8, pack_obs_and_next_obs=True)
            for k in keys:
                rec[f"obs_{k}_{n}"] = np.asarray(rb["observations"][k])
            rec[f"rewards_{n}"] = np.asarray(rb["rewards"])
    _save("live_replay_packed.npz", rec)
    # plain ReplayBuffer (replay_buffer.py:40-75)
    Ref = ref_shim.load_reference_plain_buffer_cls()
    S, A, cap = 7, 3, 41
    ref = Ref(ref_shim.Box(-np.inf, np.inf, (S,), np.float32), ref_shim.Box(-1, 1, (A,), np.float32), cap)
    ref.seed(5)
    rec = {}
    for i, tr in enumerate(itertools.islice(flat_stream(S, A, 6, 99), 100)):
        ref.insert(tr)
        if i % 17 == 16:
            b = ref.sample(13)
            for f in ("observations", "next_observations", "actions", "rewards", "masks", "dones"):
                rec[f"{f}_{i}"] = np.asarray(b[f])
    _save("live_replay_plain.npz", rec)


def populate_data_store():
    """data/data_store.py populate_data_store / populate_data_store_with_z_axis_only (the module imports agentlace, which is
    not installed; these functions only need pickle / numpy / copy) on the demo files of tests/test_host_logic.py."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pathlib
    from test_host_logic import _demo_files, _ListStore
    names = ["populate_data_store", "populate_data_store_with_z_axis_only"]
    path = os.path.join(ref_shim.REFERENCE_ROOT, "serl_launcher", "data", "data_store.py")
    tree = ast.parse(open(path).read())
    mod = ast.Module([n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names], type_ignores=[])
    ns = {"DataStoreBase": object}
    exec(compile(mod, path, "exec"), ns)
    rec = {}
    with tempfile.TemporaryDirectory() as d:
        paths = _demo_files(pathlib.Path(d))
        for name in names:
            st = _ListStore()
            ns[name](st, paths)
            rec[name] = st.items
    with open(os.path.join(HERE, "live_populate_data_store.pkl"), "wb") as fh:
        pickle.dump(rec, fh, protocol=4)
    print("live_populate_data_store.pkl")


if __name__ == "__main__":
    assert ref_shim.reference_available() and RS.reference_available(), "the reference checkout is not present"
    update_runs()
    param_tree()
    random_crop()
    replay_buffers()
    populate_data_store()
