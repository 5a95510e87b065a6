"""GPU: the image-only behaviour-cloning agent (serl_bc_opts.no_proprio; BCAgent.create(use_proprio=False)) against the fp64
statement of tests/image_only_bc.py with injected Dropout masks, at the bounds of tests/test_learner_regimes_gpu.py (info scalars and
every gradient leaf through the step-1 moments at 1e-4, head columns against the float32 oracle's error) and of tests/test_bc_gpu.py
(parameters after two steps, inference); the state dict round trip, the refusals across the two kinds, NaN states and NULL state
pointers."""
import ctypes as C

import numpy as np
import pytest
import torch

import bc_oracle as BO
import image_only_bc as IB
import learner_regimes as LR
from test_bc_gpu import LR as ADAM_LR, TOL, _close
from test_chain_fusion_gpu import _bits_equal
from test_learner_regimes_gpu import _check_bc_step

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _statement():
    with IB.installed():
        yield


def _obs(inp):
    obs = {k: torch.tensor(v[:, None], device="cuda") for k, v in inp["frames"].items()}
    obs["state"] = torch.tensor(inp["state"], device="cuda")
    return obs


def _bits(agent):
    return {(sec, leaf): agent.get(sec, leaf).copy() for leaf in agent.leaves(trainable=True) for sec in ("params", "opt/mu", "opt/nu")}


@pytest.mark.parametrize("case", IB.CASES, ids=IB.IDS)
def test_two_updates_and_inference_match_the_statement(gpu, case):
    r64, r32 = IB.run(case), IB.run(case, torch.float32)
    cfg, B = r64["cfg"], r64["B"]
    agent = IB.bc_agent(cfg, B, r64["trunk"], r64["theta"])
    assert agent.use_proprio is False and int(agent.L.serl_bc_use_proprio(agent._h)) == 0
    assert sorted(agent.leaves(trainable=True)) == sorted(IB.TRAIN) and not any(k.startswith("enc/proprio") for k in agent._counts)
    assert agent._counts["actor/w1"] == 256 * cfg.n_cam * 256
    for i, (s64, s32) in enumerate(zip(r64["steps"], r32["steps"])):
        inp = s64["inp"]
        _, info = agent.update(LR.bc_batch(inp["frames"], inp["state"], inp["action"]), masks=inp["masks"])
        info = dict(info)
        if i == 0:
            _check_bc_step(f"image-only bc {case[0]}", cfg, agent, info, s64, s32)
        for k, ref in s64["info"].items():
            assert abs(info[k] - ref) / max(1.0, abs(ref)) < TOL, (i, k, info[k], ref)
    st = r64["state"]
    assert agent.state.step == st.step == 2
    for leaf in IB.TRAIN:                    # tests/test_bc_gpu.py::_check_state's rules
        for sec, ref in (("params", st.params[leaf]), ("opt/mu", st.mu[leaf]), ("opt/nu", st.nu[leaf])):
            got, ref = agent.get(sec, leaf).astype(np.float64), ref.numpy().reshape(-1)
            e, scale = np.abs(got - ref), np.abs(ref).max() + 1e-300
            if sec == "params":
                assert np.percentile(e / scale, 99.9) < TOL and e.max() <= 2 * ADAM_LR * 2 + TOL * scale, (leaf, e.max(), scale)
            else:
                assert e.max() / scale < TOL, (sec, leaf, e.max() / scale)
    inf = IB.inputs(cfg, B, 90)
    feats = BO.features(r64["trunk"], cfg, inf["frames"])
    _close(agent.sample_actions(_obs(inf), argmax=True), BO.sample_actions(st, feats, inf["state"]).numpy())
    got = agent.get_debug_metrics(LR.bc_batch(inf["frames"], inf["state"], inf["action"]))
    for k, ref in BO.debug_metrics(st, feats, inf["state"], inf["action"]).items():
        _close(got[k], ref.numpy())


def test_nan_states_and_null_state_pointers_change_nothing(gpu):
    case = IB.CASES[1]
    r = IB.run(case)
    cfg, B = r["cfg"], r["B"]
    inp = r["steps"][0]["inp"]
    res = []
    for mode in ("state", "nan", "null"):
        agent = IB.bc_agent(cfg, B, r["trunk"], r["theta"])
        state = np.full_like(inp["state"], np.nan) if mode == "nan" else inp["state"]
        db = agent.prepare(LR.bc_batch(inp["frames"], state, inp["action"]))
        if mode == "null":
            db.cstruct.state = None
        _, info = agent.update(db, masks=inp["masks"])
        out = torch.empty((B, cfg.A), dtype=torch.float32, device="cuda")
        frames = db.frames[0].contiguous()
        sp = None if mode == "null" else C.c_void_p(db.state[0].data_ptr())
        assert agent.L.serl_bc_sample_actions(agent._h, C.c_void_p(frames.data_ptr()), sp, B, None, None, 1.0, 1, C.c_void_p(out.data_ptr()), agent._stream()) == 0
        m = agent.get_debug_metrics(db)
        res.append((_bits(agent), dict(info), out.cpu().numpy(), m))
        assert all(np.isfinite(v) for v in res[-1][1].values()) and np.isfinite(res[-1][2]).all() and all(np.isfinite(v).all() for v in m.values())
    for other in res[1:]:
        assert other[1] == res[0][1] and _bits_equal(other[2], res[0][2])
        for key, v in other[0].items():
            assert _bits_equal(v, res[0][0][key]), key
        for k, v in other[3].items():
            assert _bits_equal(v, res[0][3][k]), k


def test_state_dict_round_trip_and_the_refusals_across_the_two_kinds(gpu):
    agent = IB.create(B=4, seed=3)                    # the reference's default: use_proprio=False
    assert agent.use_proprio is False and agent.config["use_proprio"] is False
    inp = IB.inputs(IB.IO.ImageOnlyConfig(image_keys=("wrist",), H=32, W=32, S=IB.S, A=3, use_proprio=False), 4, 5)
    for _ in range(2):
        agent.update(LR.bc_batch(inp["frames"], inp["state"], inp["action"]))
    sd = agent.state.state_dict()
    enc = sd["params"]["modules_actor"]["encoder"]
    assert sorted(enc) == ["encoder_wrist"] and sd["params"]["modules_actor"]["network"]["Dense_0"]["kernel"].shape == (256, 256)
    fresh = IB.create(B=4, seed=9)
    fresh.state.load_state_dict(sd)
    assert fresh.state.step == agent.state.step == 2
    want = _bits(agent)
    for key, v in _bits(fresh).items():
        assert _bits_equal(v, want[key]), key
    agent.update(LR.bc_batch(inp["frames"], inp["state"], inp["action"]))
    fresh.update(LR.bc_batch(inp["frames"], inp["state"], inp["action"]))
    want = _bits(agent)
    for key, v in _bits(fresh).items():
        assert _bits_equal(v, want[key]), ("after the next update", key)
    prop = IB.create(B=4, seed=3, use_proprio=True)
    assert "enc/proprio/dense/kernel" in prop._counts and prop._counts["actor/w1"] == 320 * 256
    for src, dst in ((agent, prop), (prop, agent)):
        before, step = _bits(dst), dst.state.step
        with pytest.raises(ValueError, match=f"use_proprio={src.use_proprio}.*this agent has use_proprio={dst.use_proprio}; nothing was loaded"):
            dst.state.load_state_dict(src.state.state_dict())
        assert dst.state.step == step
        for key, v in _bits(dst).items():
            assert _bits_equal(v, before[key]), ("touched by the refused restore", key)


# ---- the reference's own code: tests/golden/imgonly_bc_64.npz ----------------------------------------------------------------------
def test_update_and_inference_match_the_reference_golden(gpu):
    """tests/test_bc_gpu.py::test_update_matches_reference_with_injected_masks / test_inference_matches_reference on the golden of
    the reference's BCAgent.create(use_proprio=False), at that file's bounds (_check_state, _close)"""
    import zlib
    from oracle.ref_update_runner import synth_packed_batch
    from test_bc_gpu import _batch, _check_state
    d, meta, cfg = IB.golden()
    B = meta["B"]
    trunk, theta = IB.theta_of(cfg, meta["param_seed"])
    agent = IB.bc_agent(cfg, B, trunk, theta)
    agent.state.replace(rng=np.asarray(meta["rng0"], np.uint32))
    for i in range(meta["steps"]):
        pb = synth_packed_batch(cfg, B, meta["batch_seed"] + i)
        for k, v in pb["frames"].items():
            assert np.uint32(zlib.crc32(v.tobytes())) == d[f"s{i}_crc_{k}"]
        _, info = agent.update(_batch(cfg, pb), masks=IB.golden_masks(d, cfg, i, B))
        ref = d[f"s{i}_info"]
        assert abs(info["actor_loss"] - ref[0]) < TOL * max(1.0, abs(ref[0])), (i, dict(info), ref)
        assert abs(info["mse"] - ref[1]) < TOL * max(1.0, abs(ref[1])), (i, dict(info), ref)
    _check_state(agent, d, meta, meta["steps"])
    pb = synth_packed_batch(cfg, B, meta["infer_seed"])
    obs = {k: torch.tensor(v[:, :1], device="cuda") for k, v in pb["frames"].items()}
    obs["state"] = torch.tensor(pb["state"], device="cuda")
    _close(agent.sample_actions(obs, argmax=True), d["inf_argmax"])
    for tag, temp in (("sample", 1.0), ("sample_t025", 0.25)):
        _close(agent.sample_actions(obs, seed=d[f"inf_{tag}_eps"].astype(np.float32), temperature=temp), d[f"inf_{tag}"])
    dbg = agent.get_debug_metrics({"observations": obs, "next_observations": {"state": obs["state"]},
                                   "actions": torch.tensor(pb["action"], device="cuda")})
    _close(dbg["pi_actions"], d["dbg_pi_actions"])
    _close(dbg["mse"], d["dbg_mse"])
    _close(dbg["log_probs"], d["dbg_log_probs"], 1e-3)
