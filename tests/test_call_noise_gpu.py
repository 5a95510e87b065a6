"""GPU: the learner's jax.random path (DataParallelLearner(device_noise="threefry"), what bench.py runs) against the agent's.

One update call draws REDQ indices, policy noise and Dropout masks from the call's keys, in the kernels ("keys") or as tensors
filled by one launch ("tensors").  The agent's path is pinned by the reference's goldens (tests/test_golden_update_gpu.py); here
the learner is held to it: from the same seed and the same replay contents it must leave the agent's bytes, and a rank of a
batch-sharded job must draw its rows of the GLOBAL arrays (tensor windows first = lo * width, count = rows * width of
n_total = global rows * width; the kernels' own draws through serl_agent_set_shard)."""
import itertools

import numpy as np
import pytest
import torch

from helpers import make_spaces
from oracle import drq_oracle as O
import agent_helpers as AH

pytestmark = pytest.mark.gpu
KEYS, H, W, S, A = ("front", "wrist"), 64, 64, 5, 3
SEED = 3
FORMS = ("keys", "tensors")
LEAVES = ("critic/w1", "actor/w2", "enc/0/dense/kernel", "temp/lagrange")


def _store():
    from serl_amd.data.data_store import MemoryEfficientReplayBufferDataStore
    from serl_amd.utils.synthetic import transition_stream
    osp, asp = make_spaces(KEYS, H, W, 3, 1, S, A)
    rb = MemoryEfficientReplayBufferDataStore(osp, asp, 200, image_keys=KEYS)
    rb.seed(0)
    for tr in itertools.islice(transition_stream(KEYS, H, W, 3, 1, S, A, 20, 1), 120):
        rb.insert(tr)
    return rb


def _agent(B):
    from serl_amd.utils.launcher import make_drq_agent
    obs = {k: np.zeros((1, H, W, 3), np.uint8) for k in KEYS}
    obs["state"] = np.zeros((1, S), np.float32)
    return make_drq_agent(SEED, obs, np.zeros((A,), np.float32), image_keys=KEYS, encoder_type="resnet-pretrained", batch_size=B)


def _learner(core, rb, B, form, rank=0, world=1, **kw):
    from serl_amd.agents.batch import DeviceBatch
    from serl_amd.data.data_store import gather_crop
    from serl_amd.parallel import DataParallelLearner
    dbs = {}

    def gather(parts, co, cn, slot):
        if slot not in dbs:
            dbs[slot] = DeviceBatch(B // world, len(KEYS), H, W, 3, S, A, 0)
        gather_crop(parts, co, cn, dbs[slot])
        return dbs[slot]

    lr = DataParallelLearner(core, gather, [rb], [B], rank, world, seed=SEED, image_keys=KEYS, device_noise="threefry", **kw)
    assert lr.device_noise == "threefry"
    lr.noise_form = form
    return lr


def _end_state(core, rng, draws):
    torch.cuda.synchronize()
    return {"draws": draws, "rng": np.array(rng), "step": core.step, "params": {leaf: core.get("params", leaf) for leaf in LEAVES}}


def _run_agent(form):
    agent, rb = _agent(8), _store()
    agent.noise_form = form
    it = rb.get_iterator(sample_args={"batch_size": 8, "pack_obs_and_next_obs": True, "lazy": True})
    draws = []
    for _ in range(2):
        agent.update_critics(next(it))
        agent.update_high_utd(next(it), utd_ratio=1)
        d = agent.last_draws
        draws.append((d["crop_obs"], d["crop_next"], d["redq_idx"]))
    return _end_state(agent.core, agent.state.rng, draws)


def _run_learner(form):
    from serl_amd.parallel import SerialSchedule
    lr = _learner(_agent(8).core, _store(), 8, form, schedule=SerialSchedule())
    draws = []
    for _ in range(2):
        lr.iteration(2)
        d = lr.last_draws
        draws.append((d["crops"][0], d["crops"][1], d["redq_idx"]))
    return _end_state(lr.core, lr._rng, draws)


@pytest.mark.parametrize("form", FORMS)
def test_learner_equals_agent_from_the_same_seed(gpu, form):
    """Two iterations of update_critics + update_high_utd(utd_ratio=1): the agent on its lazy iterator, then the learner on the
    core of an identical second agent.  Same crop offsets, REDQ indices, state.rng and -- bit for bit -- parameters.
    (One side runs to its end before the other starts: trunk passes of two handles that overlap on two streams do not both
    take the fused GroupNorm epilogues -- trunk_f16x3.hip claim_fused_pass -- and the other path rounds differently.)"""
    a, l = _run_agent(form), _run_learner(form)
    for i, (da, dl) in enumerate(zip(a["draws"], l["draws"])):
        assert np.array_equal(da[0], dl[0]) and np.array_equal(da[1], dl[1]), (i, "crop offsets")
        assert np.array_equal(da[2], dl[2]), (i, "REDQ indices", da[2], dl[2])
    assert np.array_equal(a["rng"], l["rng"]), "state.rng"
    assert a["step"] == l["step"] == 6
    for leaf in LEAVES:
        assert np.array_equal(a["params"][leaf], l["params"][leaf]), (leaf, AH.rel_err(a["params"][leaf], l["params"][leaf]))


def _critic_grads(world, form):
    """-> [rank's critic gradient after one update_critics over a global batch of 16], a fresh agent and store per rank"""
    sl, _ = AH.leaf_slices(O.Config(image_keys=KEYS, H=H, W=W, S=S, A=A))
    n = sl["enc/proprio/ln/bias"][1]
    out = []
    for rank in range(world):
        core = _agent(16 // world).core
        lr = _learner(core, _store(), 16, form, rank, world, all_reduce=lambda t: None)
        lr.update_critics()
        torch.cuda.synchronize()
        out.append(core.debug("g_critic", n).astype(np.float64))
    return out


@pytest.fixture(scope="module")
def full_grad(gpu):
    """the one-rank critic gradient, per noise form"""
    return {form: _critic_grads(1, form)[0] for form in FORMS}


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("world", (1, 2, 4))
def test_sharded_draws_are_the_global_draws(gpu, full_grad, world, form):
    """Every rank draws, for its rows, what the single rank draws for them: the shard gradients (each normalised by the global
    batch) sum to the full-batch gradient, at the bound test_device_noise_is_indexed_by_the_global_sample uses for hashed noise."""
    full = full_grad[form]
    assert np.abs(full).max() > 0
    err = AH.rel_err(sum(_critic_grads(world, form)), full)
    print(f"world {world}, {form}: sum of shard gradients vs one rank: rel err {err:.2e}")
    assert err < 1e-5


def test_noise_forms_give_bit_equal_gradients(gpu, full_grad):
    assert np.array_equal(full_grad["keys"], full_grad["tensors"])
