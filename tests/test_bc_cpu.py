"""CPU: behaviour cloning (serl_amd.agents.bc) against tests/golden/bc_*.npz, written by tests/golden/make_golden_bc.py from the
reference's own make_bc_agent / BCAgent under oracle/jaxshim (fp64).
  - the flax paths and shapes of the BC tree equal those of the reference's BCAgent.state.params;
  - the key schedule of an update (state.rng -> new rng, loss key, per-camera Dropout key -> keep-masks) reproduces the threefry
    golden's masks and final state.rng bit for bit, with the library's host functions only;
  - an fp64 NumPy restatement of the no-LayerNorm tanh MLP and the diagonal-Gaussian NLL head, from the recorded encoder output,
    reproduces the golden's actor_loss, mse and the first Adam moments (0.1 x gradient) of the MLP and head leaves."""
import json
import os

import numpy as np
import pytest

from oracle import drq_oracle as O
from oracle import golden_update as G

HERE = os.path.dirname(os.path.abspath(__file__))
TRAIN = ("enc/proprio/dense/kernel", "enc/proprio/dense/bias", "enc/proprio/ln/scale", "enc/proprio/ln/bias",
         "actor/w1", "actor/b1", "actor/w2", "actor/b2", "actor/mean/kernel", "actor/mean/bias",
         "actor/logstd/kernel", "actor/logstd/bias")


def _golden(name):
    d = np.load(os.path.join(HERE, "golden", f"{name}.npz"))
    meta = json.loads(str(d["meta"]))
    return d, meta, G.cfg_from_dict(meta["cfg"])


def _flat_shapes(tree, prefix=()):
    if isinstance(tree, dict):
        out = {}
        for k, v in tree.items():
            out.update(_flat_shapes(v, prefix + (k,)))
        return out
    return {"/".join(prefix): tuple(tree)}


@pytest.mark.parametrize("name", ["bc_64", "bc_one_cam", "bc_128", "bc_84"])
def test_bc_tree_paths_and_shapes_match_reference(name):
    from serl_amd.agents.flax_tree import bc_paths, bc_shapes
    d, meta, cfg = _golden(name)
    paths, shapes = bc_paths(cfg.image_keys), bc_shapes(cfg.image_keys, cfg.H, cfg.W, cfg.S, cfg.A)
    ours = {"/".join(p): tuple(shapes[leaf]) for leaf, p in paths.items()}
    assert sorted(ours) == sorted(meta["param_paths"])
    assert ours == _flat_shapes(meta["param_tree"])
    # optax.adam(lr): (ScaleByAdamState(count, mu, nu), EmptyState()) over the whole tree, info {actor_loss, mse}
    assert meta["opt_state"] == [{"type": "ScaleByAdamState", "fields": ["count", "mu", "nu"]}, {"type": "EmptyState", "fields": []}]
    assert meta["info_keys"] == ["actor_loss", "mse"]
    assert set(TRAIN) <= set(paths)


def _bernoulli_keep(key, rows, p):
    """jax.random.bernoulli(key, p, (rows, 4096)) from jax.random.bits: uniform = bits -> [1, 2) - 1 (23 mantissa bits)"""
    from serl_amd import jaxrng as J
    bits = J.random_bits(key, rows * 4096).astype(np.uint32)
    u = ((bits >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1.0)
    return (u < np.float32(p)).reshape(rows, 4096).astype(np.uint8)


def test_bc_key_schedule_matches_threefry_golden():
    from serl_amd import jaxrng as J
    d, meta, cfg = _golden("bc_64_threefry")
    assert meta["prng"] == "threefry"
    B = meta["B"]
    # BCAgent.create: rng = PRNGKey(seed); rng, init_rng = split(rng); rng, create_rng = split(rng)  (make_bc_agent(seed=0))
    rng = J.split(J.split(J.prngkey(0))[0])[1]
    assert [int(v) for v in rng] == meta["rng0"]
    for i in range(meta["steps"]):
        new_rng, k = J.split(rng)          # common.py:197-200 (apply_loss_fns)
        key = J.split(k)[1]                # bc.py:46
        for cam in cfg.image_keys:
            ck = J.flax_make_rng(key, J.dropout_path(cam))
            want = np.unpackbits(d[f"s{i}_mask_{cam}"])[:B * 4096].reshape(B, 4096)
            assert np.array_equal(_bernoulli_keep(ck, B, 1 - cfg.dropout), want), (i, cam)
        rng = new_rng
    assert [int(v) for v in rng] == meta["rng_final"]


def _np_bc(theta, enc, act, std_min=1e-5, std_max=5.0):
    """bc.py:44-60 in fp64: MLP(Dense -> tanh, twice; no LayerNorm) -> Dense_0 mean, Dense_1 log-std; actor_loss =
    -mean_b sum_a log N(act | mean, clip(exp(log_std))); mse = mean_b sum_a (mean - act)^2.  Returns the loss, mse and the
    gradients of the loss wrt the MLP / head leaves and the proprio code."""
    f64 = lambda k: np.asarray(theta[k], np.float64)  # noqa: E731
    B = enc.shape[0]
    h1 = np.tanh(enc @ f64("actor/w1") + f64("actor/b1"))
    h2 = np.tanh(h1 @ f64("actor/w2") + f64("actor/b2"))
    mean = h2 @ f64("actor/mean/kernel") + f64("actor/mean/bias")
    ls = h2 @ f64("actor/logstd/kernel") + f64("actor/logstd/bias")
    raw = np.exp(ls)
    std = np.clip(raw, std_min, std_max)
    z = (act - mean) / std
    lp = (-0.5 * z ** 2 - np.log(std) - 0.5 * np.log(2 * np.pi)).sum(-1)
    loss, mse = -lp.mean(), ((mean - act) ** 2).sum(-1).mean()
    dmean = -(z / std) / B
    dls = np.where((raw > std_min) & (raw < std_max), -(z ** 2 - 1.0) / B, 0.0)
    g = {"actor/mean/kernel": h2.T @ dmean, "actor/mean/bias": dmean.sum(0),
         "actor/logstd/kernel": h2.T @ dls, "actor/logstd/bias": dls.sum(0)}
    dh2 = dmean @ f64("actor/mean/kernel").T + dls @ f64("actor/logstd/kernel").T
    d2 = dh2 * (1 - h2 ** 2)
    g["actor/w2"], g["actor/b2"] = h1.T @ d2, d2.sum(0)
    d1 = (d2 @ f64("actor/w2").T) * (1 - h1 ** 2)
    g["actor/w1"], g["actor/b1"] = enc.T @ d1, d1.sum(0)
    return loss, mse, g


@pytest.mark.parametrize("name", ["bc_64", "bc_one_cam", "bc_84"])
def test_numpy_restatement_reproduces_golden_loss_and_gradients(name):
    from oracle.ref_update_runner import synth_packed_batch
    d, meta, cfg = _golden(name)
    assert meta["steps"] == 1 and meta["final_step"] == 1
    _, theta = O.init_params(cfg, meta["param_seed"])
    pb = synth_packed_batch(cfg, meta["B"], meta["batch_seed"])
    loss, mse, g = _np_bc(theta, d["enc0"], pb["action"].astype(np.float64))
    info = d["s0_info"]
    assert abs(loss - info[0]) < 1e-9 * max(1.0, abs(info[0])), (loss, info)
    assert abs(mse - info[1]) < 1e-9 * max(1.0, abs(info[1])), (mse, info)
    for leaf, grad in g.items():   # after one optax.adam step mu = (1 - b1) g exactly
        rec = {k.split("|")[2]: d[k] for k in d.files if k.startswith(f"f_mu|{leaf}|")}
        err, _ = G.leaf_compare(f"mu/{leaf}", rec, 0.1 * grad)
        assert err < 1e-9, (leaf, err)
