"""CPU: pins oracle/drq_oracle.py against the REFERENCE's own update code.

* golden fixtures tests/golden/update_*.npz were produced by tests/golden/make_golden_update.py, which imports the
  reference's DrQAgent (agents/continuous/drq.py:255-328 -> sac.py:243-299,544-596 -> common/common.py:124-221) from
  /root/reference and runs it UNMODIFIED, in fp64, under stand-ins for its absent third-party libraries
  (oracle/jaxshim).  The oracle, fed the noise that run drew, must reproduce every info scalar and the whole final
  train state (params, target params, all three Adam states) to fp64 round-off.
* tests/golden/live_*.{npz,json} were produced by tests/golden/make_golden_live.py from further runs of the reference's own code
  (one update schedule per random stream, its random crop, its parameter tree); the tests below compare the oracle with them.
"""
import glob
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from oracle import drq_oracle as O
from oracle import golden_update as G
from oracle import ref_update_runner as RR

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "update_*.npz")))
F64_TOL = 1e-9


def _run_oracle(cfg, steps, param_seed):
    trunk, theta = O.init_params(cfg, param_seed)
    st = O.TrainState(cfg, trunk, theta, torch.float64)
    return st, RR.run_steps(st, steps, torch.float64)


def _oracle_sections(st):
    secs = {"params": st.params, "target": st.target}
    for tx in O.TX_NAMES:
        secs[f"mu_{tx}"], secs[f"nu_{tx}"] = st.opt[tx]["mu"], st.opt[tx]["nu"]
    return secs


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[7:-4] for p in GOLDEN])
def test_oracle_reproduces_the_reference_golden(path):
    g = G.unpack(np.load(path))
    cfg = g["cfg"]
    st, infos = _run_oracle(cfg, g["steps"], g["meta"]["param_seed"])
    sched = O.TrainState(cfg, {}, {}, torch.float64)
    st_counts, c = [], 0
    for step in g["steps"]:       # optimizer count before the LAST optimizer step of each call
        c += {"critics": 1, "update": 1}.get(step["kind"], step["utd"] + 1)
        st_counts.append(c - 1)
    for i, (info, step) in enumerate(zip(infos, g["steps"])):
        for k, v in info.items():
            r = step["info"][k]
            assert abs(v - r) <= F64_TOL * max(1.0, abs(r)), (i, k, v, r)
        # the reference logs the (float32) learning rate each optimizer used: schedule(count before the step)
        count = st_counts[i]
        for tx in O.TX_NAMES:
            assert abs(step["info"][f"{tx}_lr"] - np.float32(sched.lr_at(count, tx))) < 1e-12, (i, tx)
    assert st.step == g["meta"]["final_step"]
    worst = 0.0
    for sec, tree in _oracle_sections(st).items():
        for name, t in tree.items():
            e, how = G.leaf_compare(f"{sec}/{name}", g["final"][sec][name], t.numpy())
            assert e < F64_TOL, (sec, name, how, e)
            worst = max(worst, e)
    print(f"{os.path.basename(path)}: oracle vs reference golden, worst {worst:.1e}")


def test_golden_fixtures_exist():
    assert len(GOLDEN) >= 8, "tests/golden/update_*.npz missing: run tests/golden/make_golden_update.py in the build container"


def test_sampled_records_hold_the_count_their_file_states():
    """every committed file written by oracle.golden_update.pack: the sample count it states (its *_n_sample key, record_form[1],
    or, where it stores none, its generator's constant) is the size of every sampled record in it -- the size the readers
    (G.leaf_compare, G.leaf_errors) draw their indices with"""
    import init_golden_helpers as IG
    seen = 0
    for path in sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "*.npz"))):
        name = os.path.basename(path)
        if not name.startswith(("update_", "init_", "live_update_", "widths_", "trained_update_", "policy_", "act_")):
            continue
        z = np.load(path)
        sizes = {k: z[k].size for k in z.files if k.endswith(("|val", "/val"))}
        if "final_index" in z.files:
            sizes.update({k: n for k, n in json.loads(str(z["final_index"])) if k.endswith("|val")})
        stated = [int(z[k]) for k in z.files if k.endswith("_n_sample")] + ([int(z["record_form"][1])] if "record_form" in z.files else [])
        stated = stated or [IG.N_SAMPLE if name.startswith("init_") else G.N_SAMPLE]
        assert len(stated) == 1 and sizes and set(sizes.values()) == {stated[0]}, (name, stated, sorted(set(sizes.values())))
        seen += 1
    assert seen >= len(GOLDEN) + 20, seen



class _Records(dict):
    """npz-like view (`.files`, `[key]`) of a live_update_*.npz with its final-state records unpacked from final_data"""
    @property
    def files(self):
        return list(self)


def _live(name):
    """A reference run recorded by tests/golden/make_golden_live.py (the reference's own update code, fp64).  Its final-state
    records use a smaller sample per leaf than oracle/golden_update.py's default: the comparison follows each record's size."""
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", f"live_update_{name}.npz"))
    rec = _Records((k, z[k]) for k in z.files if k not in ("final_index", "final_data"))
    data, at = z["final_data"], 0
    for key, n in json.loads(str(z["final_index"])):
        rec[key] = data[at:at + n]
        at += n
    assert at == data.size
    return G.unpack(rec), rec


def _assert_final_state(st, g, sections=None):
    for sec, tree in _oracle_sections(st).items():
        if sections is not None and sec not in sections:
            continue
        assert set(g["final"][sec]) == set(tree), sec
        for name, t in tree.items():
            e, how = G.leaf_compare(f"{sec}/{name}", g["final"][sec][name], t.numpy())
            assert e <= F64_TOL, (sec, name, how, e)


def test_live_reference_matches_oracle():
    """A reference run (peg-insertion key names / dims, critics / high_utd(2) / critics) against the oracle: every info
    scalar, the optimizer counts and the whole final train state."""
    g, z = _live("peg")
    cfg = g["cfg"]
    assert cfg.image_keys == ("wrist_1", "wrist_2") and (cfg.H, cfg.W, cfg.S, cfg.A) == (64, 64, 19, 7) and g["B"] == 4
    assert [s["kind"] for s in g["steps"]] == ["critics", "high_utd", "critics"]
    st, infos = _run_oracle(cfg, g["steps"], 7)
    for info, step in zip(infos, g["steps"]):
        assert set(info) <= set(step["info"])
        for k, v in info.items():
            assert abs(v - step["info"][k]) <= F64_TOL * max(1.0, abs(step["info"][k])), (k, v, step["info"][k])
    assert st.step == g["meta"]["final_step"] == 5 and all(tuple(c) == (5, 5) for c in z["count"])
    _assert_final_state(st, g)
    # frozen trunk: parameters untouched, target copy = EMA of identical values (drifts by round-off only)
    trunk, _ = O.init_params(cfg, 7)
    mine = np.ascontiguousarray(trunk["trunk/conv_init"].astype(np.float64).reshape(-1))
    assert hashlib.sha256(mine.tobytes()).hexdigest() == str(z["trunk_conv_init_sha256"])
    assert float(z["trunk_conv_init_target_drift"]) < 1e-14


def test_live_reference_on_jax_key_chain():
    """The same with the stand-in jax.random drawing through JAX's own threefry2x32 key chain (oracle/jaxshim/jax/threefry.py,
    pinned in tests/test_threefry_oracle.py): the reference's split / fold_in / randint / normal / bernoulli calls then consume
    the numbers a real JAX run draws for these keys; the oracle, fed the recorded draws, still agrees."""
    g, _ = _live("key_chain")
    cfg = g["cfg"]
    assert g["meta"]["prng"] == "threefry" and cfg.image_keys == ("front",) and (cfg.S, cfg.A) == (7, 4)
    st, infos = _run_oracle(cfg, g["steps"], 3)
    for info, step in zip(infos, g["steps"]):
        for k, v in info.items():
            assert abs(v - step["info"][k]) <= F64_TOL * max(1.0, abs(step["info"][k])), (k, v, step["info"][k])
    _assert_final_state(st, g, sections=("params",))


def test_reference_random_crop_equals_the_oracle_shift():
    """vision/data_augmentations.py:7-36 (edge pad 4 + dynamic_slice) as the reference computed it == oracle random_shift."""
    from oracle.replay_oracle import random_shift
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "live_random_crop.npz"))
    img = np.random.default_rng(0).integers(0, 256, (6, 1, 24, 20, 3), dtype=np.uint8)
    out, offs = z["out"], z["offs"]
    assert out.shape == img.shape
    assert offs.shape == (6, 2) and offs.min() >= 0 and offs.max() <= 8
    assert np.array_equal(out[:, 0], random_shift(img[:, 0], offs))


def test_reference_parameter_tree_is_what_the_product_exports():
    """agent.state.params of the reference (built by its own make_drq_agent + load_resnet10_params on a synthetic
    pickle) has exactly the paths serl_amd/agents/flax_tree.py exports, the trunk only under the first camera."""
    from serl_amd.agents import flax_tree as FT
    cfg = O.Config(image_keys=("front", "wrist"), H=64, W=64, S=5, A=3)
    with open(os.path.join(os.path.dirname(__file__), "golden", "live_param_tree.json")) as fh:
        tree = json.load(fh)

    def paths(t, pre=()):
        out = {}
        for k, v in t.items():
            if isinstance(v, dict):
                out.update(paths(v, pre + (k,)))
            else:
                out[pre + (k,)] = tuple(v)
        return out

    ref_paths = paths(tree)
    mine = {}
    shapes = FT.theta_shapes(2, 64, 64, 5, 3)
    for leaf, ps in FT.theta_paths(cfg.image_keys).items():
        mine[ps[0]] = tuple(shapes[leaf])
    tsh = FT.trunk_shapes()
    for leaf, sub in FT._trunk_paths().items():
        mine[("modules_actor", "encoder", f"encoder_{FT.trunk_owner(cfg.image_keys)}", "pretrained_encoder") + sub] = tuple(tsh[leaf])
    assert set(mine) == set(ref_paths), (sorted(set(mine) ^ set(ref_paths))[:6])
    for p, shp in mine.items():
        assert int(np.prod(shp)) == int(np.prod(ref_paths[p])), (p, shp, ref_paths[p])
