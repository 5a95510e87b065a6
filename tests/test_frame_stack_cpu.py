"""CPU: frame-stacked observations (num_stack = T > 1) for the SmallEncoder DrQ learner.

* tests/golden/stack2_update_drq_small.npz is a run of the REFERENCE's own DrQAgent at T = 2 (made by
  tests/golden/make_golden_update_stacked.py); oracle/drq_oracle.py, widened by tests/stacked_oracle.py and fed channel-folded
  frames, must reproduce it at the float64 tolerance tests/test_reference_update.py uses for update_drq_small_encoder.
* the B*T crop offsets per stream and state.rng come out of the library's host key schedule bit for bit;
* param_init="reference" at T = 2 equals the parameters the reference's model_def.init drew (the golden's params0), bit for bit;
* the header, the ctypes tables and the built library agree on the additions (num_stack in serl_batch and serl_agent_cfg,
  serl_crop_packed_stacked)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import drq_oracle as O
from oracle import ref_update_runner as RR
import stacked_oracle as SO
from test_reference_update import F64_TOL


@pytest.fixture(scope="module")
def golden():
    return SO.unpack(np.load(SO.golden_path()))


def test_golden_is_a_stack_of_two(golden):
    g = golden
    assert g["T"] == 2 and g["B"] == 6 and g["cfg"].image_keys == ("front", "wrist") and (g["cfg"].H, g["cfg"].W) == (64, 64)
    assert g["cfg"].S == 2 * 5 and g["cfg"].A == 3 and g["cfg"].small and g["meta"]["prng"] == "threefry"
    assert [s["kind"] for s in g["steps"]] == ["critics", "high_utd", "update", "critics"] and g["steps"][1]["utd"] == 2
    enc = g["meta"]["param_tree"]["modules_actor"]["encoder"]
    assert enc["encoder_front"]["Conv_0"]["kernel"] == [3, 3, 6, 32] and enc["Dense_0"]["kernel"] == [10, 64]
    for i in (0, 1, 3):     # B*T offsets per stream, and the frames of a stack do not share one
        co = g["steps"][i]["noise"]["crop_obs"]
        assert co.shape == (12, 2) and g["steps"][i]["noise"]["crop_next"].shape == (12, 2)
        assert any(not np.array_equal(co[2 * b], co[2 * b + 1]) for b in range(6))
    assert os.path.getsize(SO.golden_path()) < (1 << 20)


def test_fp64_restatement_reproduces_the_reference_at_num_stack_2(golden):
    g = golden
    cfg, T = g["cfg"], g["T"]
    st = SO.train_state(cfg, T, g["meta"]["param_seed"])
    def folded(cfg, step, dtype):      # channel-folded frames, cropped with the step's B*T offsets per stream
        n = step["noise"]
        fr = SO.cropped(cfg, T, step["batch"], n.get("crop_obs"), n.get("crop_next"))
        return SO.oracle_batch(cfg, T, step["batch"], fr), O.noise_to_torch(n, dtype)

    def check(i, step, info):
        for k, v in info.items():
            r = step["info"][k]
            assert abs(v - r) <= F64_TOL * max(1.0, abs(r)), (i, k, v, r)
    RR.run_steps(st, g["steps"], torch.float64, on_info=check, inputs=folded)
    assert st.step == g["meta"]["final_step"] == 6
    secs = {"params": st.params, "target": st.target}
    for tx in O.TX_NAMES:
        secs[f"mu_{tx}"], secs[f"nu_{tx}"] = st.opt[tx]["mu"], st.opt[tx]["nu"]
    worst = 0.0
    for sec, tree in secs.items():
        for name, t in tree.items():
            e = SO.leaf_compare(f"{sec}/{name}", g["final"][sec][name], t.numpy())
            assert e < F64_TOL, (sec, name, e)
            worst = max(worst, e)
    print(f"stacked oracle vs reference golden (T = 2): worst {worst:.1e}")


def test_host_draw_gives_the_goldens_crop_offsets_and_rng(golden):
    from serl_amd import jaxrng as J
    g = golden
    T, B = g["T"], g["B"]
    rng = np.asarray(g["meta"]["rng0"], np.uint32)
    assert np.array_equal(rng, J.create_rng(0))
    for step in g["steps"]:
        if step["kind"] == "update":        # SACAgent.update: no augmentation split
            keys = J.UpdateKeys(rng, False, 1, True, True)
        else:
            co, cn = J.crop_pair(rng, B * T)
            assert co.dtype == np.int32 and co.shape == (B * T, 2)
            assert np.array_equal(co, step["noise"]["crop_obs"]) and np.array_equal(cn, step["noise"]["crop_next"])
            keys = J.UpdateKeys(rng, True, step["utd"], step["kind"] == "high_utd")
        rng = keys.rng_out
    assert [int(v) for v in rng] == g["meta"]["rng_final"]


def test_reference_param_init_at_num_stack_2_equals_the_goldens_params0(golden):
    from serl_amd.utils import init_ref as IR
    g = golden
    cfg, T = g["cfg"], g["T"]
    got = IR.theta_reference(cfg.image_keys, cfg.H, cfg.W, cfg.S, cfg.A, 0, ensemble=cfg.ensemble, encoder_type="small",
                             temperature_init=1e-2, device=None, num_stack=T)
    assert got["enc/0/conv0/kernel"].shape == (3, 3, 3 * T, 32) and got["enc/proprio/dense/kernel"].shape == (cfg.S, 64)
    recs = {SO.product_name(k, cfg.image_keys): (k, v) for k, v in g["final"]["params0"].items()}
    assert set(recs) == set(got)
    for name, (gname, rec) in recs.items():
        v = np.asarray(got[name], np.float32).reshape(-1)
        if "full" in rec:
            want, have = rec["full"].astype(np.float32), v
        else:
            want, have = rec["val"].astype(np.float32), v[SO._sample_idx(v.size, SO.G._salt(f"params0/{gname}"))]
            st = np.array([v.astype(np.float64).sum(), (v.astype(np.float64) ** 2).sum()])
            assert np.allclose(st, rec["stat"][:2], rtol=1e-9, atol=1e-9), (name, st, rec["stat"][:2])
        assert have.shape == want.shape and np.array_equal(have.view(np.uint32), want.view(np.uint32)), name


def test_numpy_param_init_draws_the_widened_leaves_with_their_fan_in():
    from serl_amd.utils import init as pinit
    th = pinit.init_theta(1, 64, 64, 3 * 7, 4, seed=1, encoder_type="small", num_stack=3)
    k = th["enc/0/conv0/kernel"]
    assert k.shape == (3, 3, 9, 32) and abs(float(k.std()) * np.sqrt(81.0) - 1) < 0.1       # lecun normal over 3*3*9
    w = th["enc/proprio/dense/kernel"]
    assert w.shape == (21, 64) and float(np.abs(w).max()) <= np.sqrt(6.0 / (21 + 64))
    assert pinit.theta_shapes(1, 64, 64, 7, 4, encoder_type="small") == pinit.theta_shapes(1, 64, 64, 7, 4, encoder_type="small", num_stack=1)


def _struct_body(name):
    from serl_amd import _lib
    txt = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "serl_mi355.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"typedef struct " + name + r"\s*\{(.*?)\}\s*" + name + r"\s*;", txt, flags=re.S)
    assert m, name
    return [d.strip() for d in m.group(1).split(";") if d.strip()]


def test_header_declares_num_stack_last_in_both_structs():
    for name in ("serl_batch", "serl_agent_cfg"):
        assert _struct_body(name)[-1] == "int num_stack", (name, _struct_body(name)[-1])


def test_library_exports_serl_crop_packed_stacked_and_the_tables_follow():
    from serl_amd import _lib, _lib_agent
    L = _lib.lib()
    assert hasattr(L, "serl_crop_packed_stacked")
    decl = _lib.exported_symbols()
    assert decl["serl_crop_packed_stacked"] == len(_lib.SIGNATURES["serl_crop_packed_stacked"]) == decl["serl_crop_packed"] + 1
    assert _lib.SerlBatch._fields_[-1] == ("num_stack", C.c_int) and _lib_agent.SerlAgentCfg._fields_[-1] == ("num_stack", C.c_int)
    assert _lib.SerlBatch().num_stack == 0 and _lib_agent.SerlAgentCfg().num_stack == 0       # zero-initialised = single frame
    # argument checks that need no device: the stack depth is refused before anything is touched
    p = (C.c_void_p * 1)(1)
    assert L.serl_crop_packed_stacked(0, p, 1, 2, 5, 32, 32, 3, None, None, C.c_void_p(1), None) == -1
    assert b"num_stack 5 not in [1,4]" in L.serl_last_error()
