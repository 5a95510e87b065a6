"""GPU: the HIP behaviour-cloning agent (csrc/bc.hip through serl_amd.agents.bc) against the reference's own BCAgent
(tests/golden/bc_*.npz, tests/golden/make_golden_bc.py, fp64 under oracle/jaxshim).
Injected-mask cases replay the keep-masks the reference drew; the threefry case draws them inside the SLE kernel from the keys
of state.rng.  Tolerances as tests/test_golden_update_gpu.py: info scalars and Adam moments 1e-4 relative to the value / the
leaf's max; parameters 99.9th percentile within 1e-4 and every element within the Adam sign-flip bound (2 lr per step)."""
import json
import os
import pickle
import zlib

import numpy as np
import pytest
import torch

from oracle import drq_oracle as O
from oracle import golden_update as G
from oracle.ref_update_runner import synth_packed_batch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TOL, LR = 1e-4, 3e-4


def _golden(name):
    d = np.load(os.path.join(HERE, "golden", f"{name}.npz"))
    meta = json.loads(str(d["meta"]))
    return d, meta, G.cfg_from_dict(meta["cfg"])


def _agent(cfg, B, meta=None):
    from serl_amd import jaxrng as J
    from serl_amd.agents.bc import BCAgent
    agent = BCAgent(cfg.image_keys, cfg.H, cfg.W, cfg.S, cfg.A, seed_key=J.prngkey(0), max_batch=B)
    trunk, theta = O.init_params(cfg, 42 if meta is None else meta["param_seed"])
    agent.load_flat(trunk)
    agent.load_flat({k: v for k, v in theta.items() if k.startswith("enc/") or k in agent._counts})
    if meta is not None:
        agent.state.replace(rng=np.asarray(meta["rng0"], np.uint32))
    return agent


def _batch(cfg, pb, dev="cuda"):
    t = lambda a: torch.tensor(a, device=dev)  # noqa: E731
    obs = {k: t(v) for k, v in pb["frames"].items()}     # packed [B, 2, H, W, 3] (pack_obs_and_next_obs=True)
    obs["state"] = t(pb["state"])
    return {"observations": obs, "next_observations": {"state": t(pb["next_state"])}, "actions": t(pb["action"]),
            "rewards": t(pb["reward"]), "masks": t(pb["mask"])}


def _masks(d, cfg, i, B):
    return {k: np.unpackbits(d[f"s{i}_mask_{k}"])[:B * 4096].reshape(B, 4096) for k in cfg.image_keys}


def _check_state(agent, d, meta, steps):
    errs = {}
    for sec, gsec in (("params", "params"), ("opt/mu", "mu"), ("opt/nu", "nu")):
        for leaf in agent.leaves(trainable=True):
            rec = {k.split("|")[2]: d[k] for k in d.files if k.startswith(f"f_{gsec}|{leaf}|")}
            assert rec, (gsec, leaf)
            got = agent.get(sec, leaf)
            if sec == "params":
                e, scale = G.leaf_errors(f"{gsec}/{leaf}", rec, got)
                assert np.percentile(e / scale, 99.9) < TOL and e.max() <= 2 * LR * steps + TOL * scale, (leaf, e.max(), scale)
            else:
                err, _ = G.leaf_compare(f"{gsec}/{leaf}", rec, got)
                assert err < TOL, (sec, leaf, err)
                errs[(sec, leaf)] = err
    assert agent.state.step == meta["final_step"] == steps
    return errs


def _frozen(agent):
    return {leaf: agent.get("params", leaf) for leaf in agent.leaves(trainable=False)}


@pytest.mark.parametrize("name", ["bc_64", "bc_one_cam", "bc_128", "bc_64_seq", "bc_84"])
def test_update_matches_reference_with_injected_masks(gpu, name):
    d, meta, cfg = _golden(name)
    B = meta["B"]
    agent = _agent(cfg, B, meta)
    before = _frozen(agent)
    for i in range(meta["steps"]):
        pb = synth_packed_batch(cfg, B, meta["batch_seed"] + i)
        for k, v in pb["frames"].items():
            assert np.uint32(zlib.crc32(v.tobytes())) == d[f"s{i}_crc_{k}"]
        _, info = agent.update(_batch(cfg, pb), masks=_masks(d, cfg, i, B))
        ref = d[f"s{i}_info"]
        assert abs(info["actor_loss"] - ref[0]) < TOL * max(1.0, abs(ref[0])), (i, info, ref)
        assert abs(info["mse"] - ref[1]) < TOL * max(1.0, abs(ref[1])), (i, info, ref)
    _check_state(agent, d, meta, meta["steps"])
    # every frozen leaf bit-identical, its moments exactly zero
    for leaf, v in _frozen(agent).items():
        assert np.array_equal(v, before[leaf]), leaf
        assert not agent.get("opt/mu", leaf).any() and not agent.get("opt/nu", leaf).any(), leaf


def test_update_threefry_masks_drawn_in_kernel(gpu):
    from serl_amd import jaxrng as J
    d, meta, cfg = _golden("bc_64_threefry")
    B = meta["B"]
    agent = _agent(cfg, B)   # state.rng from the seed alone, as make_bc_agent(0, ...) leaves it
    assert [int(v) for v in agent.state.rng] == meta["rng0"]
    assert [int(v) for v in J.split(J.split(J.prngkey(0))[0])[1]] == meta["rng0"]
    for i in range(meta["steps"]):
        _, info = agent.update(_batch(cfg, synth_packed_batch(cfg, B, meta["batch_seed"] + i)))
        ref = d[f"s{i}_info"]
        assert abs(info["actor_loss"] - ref[0]) < TOL * max(1.0, abs(ref[0])), (i, info, ref)
        assert abs(info["mse"] - ref[1]) < TOL * max(1.0, abs(ref[1])), (i, info, ref)
    _check_state(agent, d, meta, meta["steps"])
    assert [int(v) for v in agent.state.rng] == meta["rng_final"]
    # the same update with the masks injected instead is bit-identical
    ag2 = _agent(cfg, B)
    for i in range(meta["steps"]):
        ag2.update(_batch(cfg, synth_packed_batch(cfg, B, meta["batch_seed"] + i)), masks=_masks(d, cfg, i, B))
    for leaf in agent.leaves(trainable=True):
        assert np.array_equal(agent.get("params", leaf), ag2.get("params", leaf)), leaf


def _close(got, ref, tol=2e-4):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = np.abs(got - ref).max() / max(1.0, np.abs(ref).max())
    assert err < tol, err


@pytest.mark.parametrize("name", ["bc_64", "bc_one_cam", "bc_64_threefry", "bc_84"])
def test_inference_matches_reference(gpu, name):
    d, meta, cfg = _golden(name)
    B = meta["B"]
    agent = _agent(cfg, B, meta)
    for i in range(meta["steps"]):
        agent.update(_batch(cfg, synth_packed_batch(cfg, B, meta["batch_seed"] + i)), masks=_masks(d, cfg, i, B))
    pb = synth_packed_batch(cfg, B, meta["infer_seed"])
    for k, v in pb["frames"].items():
        assert np.uint32(zlib.crc32(v.tobytes())) == d[f"inf_crc_{k}"]
    obs = {k: torch.tensor(v[:, :1], device="cuda") for k, v in pb["frames"].items()}
    obs["state"] = torch.tensor(pb["state"], device="cuda")
    mode = agent.sample_actions(obs, argmax=True)
    _close(mode, d["inf_argmax"])                     # the mean, no tanh
    for tag, temp in (("sample", 1.0), ("sample_t025", 0.25)):
        _close(agent.sample_actions(obs, seed=d[f"inf_{tag}_eps"].astype(np.float32), temperature=temp), d[f"inf_{tag}"])
        if meta["prng"] == "threefry":     # the seed key itself: eps = jax.random.normal(seed, (B, A)) drawn in the kernel
            _close(agent.sample_actions(obs, seed=d["inf_key"], temperature=temp), d[f"inf_{tag}"])
    dbg = agent.get_debug_metrics({"observations": obs, "next_observations": {"state": obs["state"]},
                                   "actions": torch.tensor(pb["action"], device="cuda")})
    _close(dbg["pi_actions"], d["dbg_pi_actions"])
    _close(dbg["mse"], d["dbg_mse"])
    _close(dbg["log_probs"], d["dbg_log_probs"], 1e-3)
    # unbatched observation (one [T=1, H, W, C] image per camera): one action
    one = {k: v[0] for k, v in obs.items()}
    _close(agent.sample_actions(one, argmax=True), d["inf_argmax"][0])


def test_populate_iterator_update_matches_direct_update(gpu, tmp_path):
    import itertools
    from serl_amd.data.data_store import MemoryEfficientReplayBufferDataStore, populate_data_store
    from serl_amd.utils.synthetic import transition_stream

    class Sp:
        def __init__(self, shape):
            self.shape = shape

    class D:
        def __init__(self, s):
            self.spaces = s

    cfg = O.Config(image_keys=("front", "wrist"), H=64, W=64, S=5, A=3)
    demos = list(itertools.islice(transition_stream(cfg.image_keys, 64, 64, 3, 1, 5, 3, 20, 1), 60))
    path = tmp_path / "demos.pkl"
    with open(path, "wb") as f:
        pickle.dump(demos, f)
    osp = D({"front": Sp((1, 64, 64, 3)), "state": Sp((1, 5)), "wrist": Sp((1, 64, 64, 3))})
    rb = MemoryEfficientReplayBufferDataStore(osp, Sp((3,)), 100, image_keys=cfg.image_keys)
    rb.seed(0)
    populate_data_store(rb, [str(path)])
    it = rb.get_iterator(sample_args={"batch_size": 8, "pack_obs_and_next_obs": True})
    batch = next(it)
    direct = {"observations": {k: v.clone() for k, v in batch["observations"].items()},
              "next_observations": {k: v.clone() for k, v in batch["next_observations"].items()},
              "actions": batch["actions"].clone(), "rewards": batch["rewards"].clone(), "masks": batch["masks"].clone()}
    a1, a2 = _agent(cfg, 8), _agent(cfg, 8)
    _, i1 = a1.update(batch)
    _, i2 = a2.update({"observations": {k: v[:, :1].clone() for k, v in direct["observations"].items() if k != "state"}
                       | {"state": direct["observations"]["state"]},
                       "next_observations": direct["next_observations"], "actions": direct["actions"]})
    assert i1["actor_loss"] == i2["actor_loss"] and i1["mse"] == i2["mse"] and np.isfinite(i1["actor_loss"])
    for leaf in a1.leaves(trainable=True):
        assert np.array_equal(a1.get("params", leaf), a2.get("params", leaf)), leaf
    # a lazily sampled batch goes through the fused gather (no crop) to the same update
    a3, a4 = _agent(cfg, 8), _agent(cfg, 8)
    rb.seed(5)
    lazy = rb.sample(8, lazy=True)
    dense = lazy.materialize()
    a3.update(lazy)
    a4.update(dense)
    for leaf in a3.leaves(trainable=True):
        assert np.array_equal(a3.get("params", leaf), a4.get("params", leaf)), leaf


def test_checkpoint_roundtrip_is_bit_exact(gpu, tmp_path):
    from serl_amd.utils.checkpoint import read_checkpoint_tree, restore_checkpoint, save_checkpoint
    d, meta, cfg = _golden("bc_64")
    B = meta["B"]
    agent = _agent(cfg, B, meta)
    agent.update(_batch(cfg, synth_packed_batch(cfg, B, meta["batch_seed"])), masks=_masks(d, cfg, 0, B))
    save_checkpoint(str(tmp_path), agent.state, step=1)
    tree = read_checkpoint_tree(str(tmp_path))
    paths = set()

    def walk(t, p=()):
        for k, v in t.items():
            if isinstance(v, dict):
                walk(v, p + (k,))
            else:
                paths.add("/".join(p + (k,)))
    walk(tree["params"])
    assert sorted(paths) == sorted(meta["param_paths"])
    assert set(tree["opt_states"]) == {"0", "1"} and set(tree["opt_states"]["0"]) == {"count", "mu", "nu"} and tree["opt_states"]["1"] == {}
    fresh = _agent(cfg, B)
    restore_checkpoint(str(tmp_path), fresh.state)
    assert fresh.state.step == 1 and np.array_equal(fresh.state.rng, agent.state.rng)
    for sec in ("params", "opt/mu", "opt/nu"):
        for leaf in agent.leaves():
            assert np.array_equal(fresh.get(sec, leaf), agent.get(sec, leaf)), (sec, leaf)


def test_make_bc_agent_surface(gpu):
    from serl_amd.agents.bc import make_bc_agent
    obs = {"image": np.zeros((1, 64, 64, 3), np.uint8), "state": np.zeros((1, 7), np.float32)}
    agent = make_bc_agent(0, obs, np.zeros((4,), np.float32), image_keys=("image",), batch_size=8)
    opt = agent.state.opt_states
    assert type(opt[0]).__name__ == "ScaleByAdamState" and type(opt[1]).__name__ == "EmptyState"
    assert int(opt[0].count) == 0 and agent.state.step == 0
    with pytest.raises(ValueError):
        make_bc_agent(0, obs, np.zeros((4,), np.float32), encoder_type="small")
