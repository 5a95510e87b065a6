"""CPU: weight_decay on agents with cameras -- the fixtures (tests/pixel_weight_decay.py) and the float64 statement the GPU tests
compare against (oracle/drq_oracle.py with TrainState.live_trunk), and the learners' checks.

* the oracle (target critic on features of the TARGET trunk, features recomputed before every optimizer step) reproduces
  every info scalar and the whole final state of each wd_*.npz -- the reference's own DrQAgent with adamw -- within the bound
  tests/test_reference_update.py holds the oracle to;
* the trunk ends where the closed form says: online (1 - sum lr wd)^n, target the EMA recursion over the critic steps, in the
  reference's recorded conv_init and in every trunk leaf of the restatement; every leaf of a pretrained fixture shrinks by 5 % and
  more, so a build that leaves the trunk alone cannot pass;
* the discriminator: the oracle with live_trunk switched off, whose target critic shares the online trunk's features, misses the last step's
  critic_loss and target_qs of the pretrained fixture by at least 100 x the GPU tolerance -- the fixtures can tell a build with
  a target-trunk pass from one without;
* DataParallelLearner refuses a live-trunk core under a schedule of more than one slot, TrunkFarmLearner refuses it outright.
"""
import os

import numpy as np
import pytest
import torch

from oracle import drq_oracle as O
from oracle import golden_update as G
from oracle import ref_update_runner as RR
import agent_helpers as AH
import golden_replay as GR
import pixel_weight_decay as PW
from serl_amd.parallel import DataParallelLearner, SerialSchedule, TrunkFarmLearner
from test_parallel_cpu import FakeBuffer, FakeCore, _tagged_gather
from test_reference_update import F64_TOL, _oracle_sections

_RUNS = {}


def _need_golden(name):
    assert os.path.exists(GR.variant_path("wd", name)), \
        f"tests/golden/wd_{name}.npz missing: run tests/golden/make_golden_update_decay.py in the build container"


def _run(g, live_trunk=None):
    """the recorded schedule through the oracle from O.init_params' leaves -> (TrainState, infos); live_trunk: None = the
    Config's own rule, False = features once per call and shared by both critics"""
    st = O.TrainState(g["cfg"], *O.init_params(g["cfg"], g["meta"]["param_seed"]), torch.float64)
    assert st.live_trunk == (not g["cfg"].small)
    if live_trunk is not None:
        st.live_trunk = live_trunk
    return st, RR.run_steps(st, g["steps"], torch.float64)


def _restated(name):
    """(golden, npz, final TrainState of the oracle, its infos), once per session"""
    if name not in _RUNS:
        _need_golden(name)
        g, meta, z = GR.load_variant("wd", name)
        assert meta["weight_decay"]["decay"] == PW.DECAY and int(z["wd_n_sample"]) == PW.GOLDEN[name][3]
        assert g["cfg"] == PW.GOLDEN[name][0] and g["B"] == PW.GOLDEN[name][1]
        assert [tuple(s) if len(s) == 1 else (s[0], tuple(s[1]) if isinstance(s[1], list) else s[1]) for s in meta["schedule"]] == \
            PW.GOLDEN[name][2]
        st, infos = _run(g)
        _RUNS[name] = (g, z, st, infos)
    return _RUNS[name]


@pytest.mark.parametrize("name", list(PW.GOLDEN))
def test_restatement_reproduces_the_reference_golden(name):
    g, _, st, infos = _restated(name)
    for i, (info, step) in enumerate(zip(infos, g["steps"])):
        assert set(info) == {k for k in step["info"] if not k.endswith("_lr")}
        for k, v in info.items():
            r = step["info"][k]
            assert abs(v - r) <= F64_TOL * max(1.0, abs(r)), (i, k, v, r)
        for tx in O.TX_NAMES:
            assert abs(step["info"][f"{tx}_lr"] - np.float32(g["cfg"].lr)) < 1e-12, (i, tx)
    assert st.step == g["meta"]["final_step"] == len(PW.optimizer_steps(PW.GOLDEN[name][2]))
    worst = 0.0
    for sec, tree in _oracle_sections(st).items():
        assert set(g["final"][sec]) == set(tree), sec
        for leaf, t in tree.items():
            e, how = G.leaf_compare(f"{sec}/{leaf}", g["final"][sec][leaf], t.numpy())
            assert e < F64_TOL, (sec, leaf, how, e)
            worst = max(worst, e)
    print(f"wd_{name}: restatement vs reference golden, worst {worst:.1e}")


@pytest.mark.parametrize("name", PW.PRETRAINED)
def test_trunk_follows_the_closed_form_and_shrinks(name):
    g, z, st, _ = _restated(name)
    cfg, sched = g["cfg"], PW.GOLDEN[name][2]
    on, tg = PW.closed_form_ratios(cfg, sched)
    n = len(PW.optimizer_steps(sched))
    assert abs(on - PW.step_factor(cfg) ** n) < 1e-15 and on <= 0.95 < tg < 1.0, (on, tg)
    trunk0, _ = O.init_params(cfg, g["meta"]["param_seed"])
    # the reference's own trunk: conv_init as the run left it, online and target
    p0 = trunk0["trunk/conv_init"].astype(np.float64).reshape(-1)
    for key, ratio in (("trunk_conv_init", on), ("trunk_conv_init_target", tg)):
        assert np.abs(z[key] - ratio * p0).max() <= 1e-12 * np.abs(p0).max(), key
    # every leaf of the restatement, and the fixture's condition: every leaf lost 5 % and more
    for k, v0 in trunk0.items():
        v0 = v0.astype(np.float64)
        scale = np.abs(v0).max()
        assert np.abs(st.trunk[k].numpy() - on * v0).max() <= 1e-12 * scale, k
        assert np.abs(st.target_trunk[k].numpy() - tg * v0).max() <= 1e-12 * scale, k
        assert (np.abs(st.trunk[k].numpy()) <= 0.95 * np.abs(v0)).all(), k
    print(f"wd_{name}: {n} steps, online trunk x {on:.6f}, target x {tg:.6f}")
    if name == "update_drq_one_cam":      # the figures of the probe the fixture was specified from
        assert abs(on - 0.913182) < 1e-6 and abs(tg - 0.999037) < 1e-6


def test_shared_features_miss_the_pretrained_golden():
    """the oracle with live_trunk off computes what a library without a target-trunk pass would: right at the first step (the
    trunks are equal), off by 1.5e-2 at the last"""
    g, _, _, _ = _restated("update_drq_one_cam")
    _, infos = _run(g, live_trunk=False)
    first, last = g["steps"][0]["info"], g["steps"][-1]["info"]
    for k in ("critic_loss", "predicted_qs", "target_qs"):
        assert abs(infos[0][k] - first[k]) <= F64_TOL * max(1.0, abs(first[k])), (k, infos[0][k], first[k])
    for k in ("critic_loss", "target_qs"):
        miss = abs(infos[-1][k] - last[k]) / max(1.0, abs(last[k]))
        print(f"shared features, last step {k}: {infos[-1][k]:.6f} vs the reference's {last[k]:.6f}: {miss:.2e}")
        assert miss >= 100 * GR.TOL, (k, infos[-1][k], last[k])


def test_small_encoder_needs_no_second_trunk():
    """no frozen leaf: the trunk is not live under the Config's own rule, and the shared-features path reproduces the SmallEncoder
    fixture"""
    g, _, _, _ = _restated("update_drq_small")
    st, infos = _run(g, live_trunk=False)
    assert not O.TrainState(g["cfg"], {}, {}).live_trunk
    for info, step in zip(infos, g["steps"]):
        for k, v in info.items():
            assert abs(v - step["info"][k]) <= F64_TOL * max(1.0, abs(step["info"][k])), (k, v, step["info"][k])


def test_all_options_at_once_run_through_the_one_update_code():
    """softplus std, swish MLPs and a decayed pretrained trunk in ONE Config (PW.COMPOSED; no recorded run covers it): every
    update kind ends finite, and the trunk leaves end at the closed form within the bound of
    test_trunk_follows_the_closed_form_and_shrinks"""
    cfg, B = PW.COMPOSED, PW.COMPOSED_ROWS
    sched = [("critics",), ("high_utd", 2), ("update", ("actor", "critic", "temperature"))]
    trunk0, theta = O.init_params(cfg, GR.PARAM_SEED)
    st = O.TrainState(cfg, trunk0, theta, torch.float64)
    assert st.live_trunk
    for i, item in enumerate(sched):
        step = {"kind": item[0], "utd": item[1] if item[0] == "high_utd" else 1, "nets": item[1] if item[0] == "update" else ()}
        b = AH.batch_to_torch(AH.synth_batch(cfg, B, seed=3 + i), torch.float64)
        n = O.noise_to_torch(O.make_noise(cfg, B, seed=7 + i, utd_ratio=step["utd"]), torch.float64)
        info, _ = RR.run_step(st, step, b, n)
        assert info and all(np.isfinite(v) for v in info.values()), (item, info)
        assert ("actor_loss" in info) == (item[0] != "critics")
    assert st.step == len(PW.optimizer_steps(sched)) == 5
    assert all(torch.isfinite(v).all() for tree in (st.params, st.target) for v in tree.values())
    on, tg = PW.closed_form_ratios(cfg, sched)
    for k, v0 in trunk0.items():
        v0 = v0.astype(np.float64)
        scale = np.abs(v0).max()
        assert np.abs(st.trunk[k].numpy() - on * v0).max() <= 1e-12 * scale, k
        assert np.abs(st.target_trunk[k].numpy() - tg * v0).max() <= 1e-12 * scale, k


# ---- the learners ----------------------------------------------------------------------------------------------------------------
class LiveCore(FakeCore):
    live_trunk = True
    device = "cpu"


class ThreeSlots(SerialSchedule):
    slots = 3


def _learner(core, schedule=None):
    bufs = [FakeBuffer(500, 0), FakeBuffer(60, 1)]
    return DataParallelLearner(core, _tagged_gather(bufs), bufs, [12, 12], 0, 1, seed=3, schedule=schedule)


def test_data_parallel_learner_takes_a_live_trunk_with_one_slot_only():
    with pytest.raises(ValueError, match="live"):
        _learner(LiveCore(), ThreeSlots())
    lr = _learner(LiveCore())                  # the serial schedule runs
    lr.update_critics()
    lr.update_high_utd()
    _learner(FakeCore(), ThreeSlots())         # and a frozen trunk may be pipelined as before


def test_the_trunk_farm_refuses_a_live_trunk():
    with pytest.raises(NotImplementedError, match="live"):
        TrunkFarmLearner(LiveCore(), None, [], [8], rank=0, world=2)
    TrunkFarmLearner(FakeCore(), None, [], [8], rank=0, world=2)
