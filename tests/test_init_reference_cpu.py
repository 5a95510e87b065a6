"""CPU: param_init="reference" (serl_amd/utils/init_ref.py, serl_jax_init_host).  The host twins of the device draws against
the parameters the reference's own create code initialises from the seed (tests/golden/init_*.npz, bit for bit), the key each
leaf is drawn under, and a float64 NumPy check of the initialisers' bounds and variances that does not rest on the restatement."""
import math

import numpy as np
import pytest

import init_golden_helpers as IG
from serl_amd import jaxrng as J
from serl_amd.agents.flax_tree import theta_paths
from serl_amd.utils import init as pinit
from serl_amd.utils import init_ref as IR


@pytest.mark.parametrize("path", IG.GOLDEN, ids=IG.case_name)
def test_host_twins_equal_the_reference_initial_params(path):
    g, cfg, recs, shapes = IG.load(path)
    case = IG.case_name(path)
    got = IG.product_leaves(case, cfg, device=None)
    assert set(got) == set(recs), (sorted(set(got) ^ set(recs)))
    bad = [m for m in (IG.mismatch(n, recs[n], got[n]) for n in sorted(recs)) if m]
    assert not bad, bad
    for n, v in got.items():
        assert tuple(v.shape) == shapes[n], (n, v.shape, shapes[n])
    if "init_rng" in g.files:      # state.rng after create: rng, init_rng = split(rng); rng, create_rng = split(rng)
        assert np.array_equal(IR.create_rng_of(0), g["init_rng"])


def test_leaves_cover_init_theta_with_its_names_and_shapes():
    for keys, etype in ((("front", "wrist"), "resnet-pretrained"), (("image",), "small"), ((), "resnet-pretrained")):
        want = pinit.theta_shapes(len(keys), 64, 64, 5, 3, encoder_type=etype)
        got = {lf.name: lf.shape for lf in IR.theta_leaves(keys, 64, 64, 5, 3, encoder_type=etype)}
        assert got == {k: tuple(v) for k, v in want.items()}
    want = {k: v.shape for k, v in pinit.init_classifier(2, 64, 64).items()}
    assert {lf.name: lf.shape for lf in IR.classifier_leaves(("a", "b"), 64, 64)} == want


def test_key_derivation_table():
    """make_rng("params") of the leaf's module: the flax path from flax_tree.theta_paths, kernel on the scope's first call and
    bias on its second; the critic ensemble's members under split(init_rng, N)[i] (not fold_in) with the same suffix."""
    keys = ("front", "wrist")
    leaves = {lf.name: lf for lf in IR.theta_leaves(keys, 64, 64, 5, 3, ensemble=10)}
    paths = theta_paths(keys)
    init_rng = IR.init_rng_of(J.prngkey(0))
    assert np.array_equal(init_rng, J.split(J.prngkey(0))[1])
    for name, lf in leaves.items():
        assert lf.path + (paths[name][0][-1],) == paths[name][0]
        assert lf.counter == (2 if name.endswith("bias") or name in ("critic/b1", "critic/b2", "actor/b1", "actor/b2") else 1)
    w1 = leaves["critic/w1"]
    assert w1.members == 10 and w1.path == ("modules_critic", "network", "Dense_0")
    k = IR.leaf_keys(w1, init_rng)
    for i in range(10):
        assert np.array_equal(k[i], J.flax_make_rng(J.split(init_rng, 10)[i], w1.path, 1))
        assert not np.array_equal(k[i], J.flax_make_rng(J.fold_in(J.flax_make_rng(init_rng, w1.path[:2], 1), i), w1.path[2:], 1))
    assert leaves["critic/head/kernel"].members == 0            # DrQ: only the critic's MLP is ensemblized
    assert leaves["enc/1/sle"].path == ("modules_actor", "encoder", "encoder_wrist", "SpatialLearnedEmbeddings_0")
    assert np.array_equal(IR.leaf_keys(leaves["actor/b1"], init_rng)[0], J.flax_make_rng(init_rng, ("modules_actor", "network", "Dense_0"), 2))
    state = {lf.name: lf for lf in IR.theta_leaves((), 0, 0, 5, 3, ensemble=4)}
    assert state["critic/head/kernel"].members == 4 and state["actor/w1"].members == 0   # state SAC ensemblizes the whole Critic
    assert [lf.init for lf in IR.theta_leaves(keys, 64, 64, 5, 3) if lf.name.startswith("enc/0/")] == \
        [IR.LECUN_NORMAL, IR.LECUN_NORMAL, IR.ZEROS, IR.ONES, IR.ZEROS]
    assert leaves["enc/proprio/dense/kernel"].init == leaves["critic/w1"].init == leaves["actor/mean/kernel"].init == IR.XAVIER_UNIFORM


def test_initialiser_bounds_and_variance_float64():
    """A sanity check independent of the restated formulas: xavier_uniform lies in +-sqrt(6 / (fan_in + fan_out)) with variance
    2 / (fan_in + fan_out); lecun_normal is a normal truncated at two standard deviations with variance 1 / fan_in."""
    key = J.prngkey(7)
    fi, fo = 582, 256
    kind, lo, hi, scale = IR._job_args(IR.XAVIER_UNIFORM, (fi, fo))
    u = J.init_host(kind, key, fi * fo, lo, hi, scale).astype(np.float64)
    a = math.sqrt(6.0 / (fi + fo))
    assert np.abs(u).max() <= a * (1 + 1e-6) and np.abs(u).max() > 0.999 * a
    assert abs(u.var() / (2.0 / (fi + fo)) - 1) < 0.01 and abs(u.mean()) < 0.01 * a
    kind, lo, hi, scale = IR._job_args(IR.LECUN_NORMAL, (fi, fo))
    t = J.init_host(kind, key, fi * fo, lo, hi, scale).astype(np.float64)
    sigma = math.sqrt(1.0 / fi) / 0.87962566103423978          # the untruncated normal's standard deviation
    assert np.abs(t).max() <= 2 * sigma * (1 + 1e-6) and np.abs(t).max() > 1.99 * sigma
    assert abs(t.var() / (1.0 / fi) - 1) < 0.01 and abs(t.mean()) < 0.01 * sigma
    frac = (np.abs(t) < sigma).mean()                           # P(|x| < 1 | |x| < 2) for a unit normal
    want = math.erf(1 / math.sqrt(2)) / math.erf(2 / math.sqrt(2))
    assert abs(frac - want) < 0.005
    n = J.init_host(J.INIT_NORMAL, key, 200000, scale=2.0).astype(np.float64)
    assert abs(n.std() / 2.0 - 1) < 0.01 and abs(n.mean()) < 0.02


def test_param_init_values():
    assert IR.check_param_init("reference") and not IR.check_param_init("numpy")
    with pytest.raises(ValueError):
        IR.check_param_init("flax")
    # log(exp(t) - 1) with every op rounded to float32, as jnp computes it: exp(0.01) rounds to 1.0100502 and the subtraction
    # keeps its rounding error, so the value differs from the float64 one in the 6th digit
    e = np.float32(math.exp(float(np.float32(1e-2))))
    assert e == np.float32(1.0100502)
    assert IR.lagrange_init(1e-2) == np.float32(math.log(float(e - np.float32(1))))
    assert abs(float(IR.lagrange_init(1e-2)) - math.log(math.exp(1e-2) - 1)) < 1e-4
