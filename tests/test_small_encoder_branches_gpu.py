"""GPU parity of the trainable SmallEncoder (serl_amd/csrc/small_encoder.hip) at every branch of its backward pass's launch plan
and away from its initialisation, against the fp64 oracle (cases, plan arithmetic and the layer-by-layer fp64 statement:
tests/small_encoder_cases.py; their conditions: tests/test_small_encoder_cases_cpu.py).

Every case runs ONE update_critics with injected noise (the actor's gradient stops at the encoder output), and checks
  * the debug tap small_plan -- [row chunks of layer 0's weight gradient, K-split of layers 1, 2, 3] as launched -- against the
    case table, which proves that the branch ran;
  * every layer's ReLU output (taps small_act0..3) against the fp64 layer;
  * every conv kernel and bias leaf of g_critic by max-norm (AH.rel_err, TOL) and element by element (AH.elem_rel_err over the
    elements above 1e-3 of the leaf's largest, bound 1e-3 as tests/test_bench_shape_gpu.py),
beside the infos, q, target_q, the encoder output, every other gradient leaf and the parameters after the step, as
tests/test_small_encoder_gpu.py does.

Branch cases: one_chunk (a single chunk of 225 rows; layer 3 with one row per camera: forward GEMM M = 1, weight-gradient GEMM
K = 1, pool over one pixel), two_chunks (an uneven last chunk), four_cams (the camera limit: per-camera strides of partials, slabs
and parameters), chunk_cap (1024 chunks of which 30 are empty; K-splits of 29 and 6), split_cap (the cap of 64 slices, the last of
135 rows; a K-split on every layer).  The halving of a K-split against the workspace needs about 65 000 layer-3 rows per camera
with four cameras: no test-sized shape reaches it, and none is tried.

Regime cases: dead_channels, flat_frames (activations exactly 0 at the `> 0` masks; bytes 0 and 255), trained_scale (kernels x 4
per layer, judged with the float32 oracle as yardstick), high_utd on dead_channels' parameters; two_shards through the phase API;
and the refusal of a fifth camera when the agent is created."""
import time

import numpy as np
import pytest
import torch

from oracle import drq_oracle as O
import agent_helpers as AH
import small_encoder_cases as SC
from test_agent_gpu import TOL, _check_grads, _compare_state

pytestmark = pytest.mark.gpu
ELEM_TOL = 1e-3          # tests/test_bench_shape_gpu.py::_assert_grads


def _make_core(name):
    cfg, B, theta, _, _ = SC.inputs(name)
    return AH.load_leaves(AH.make_core(cfg, B), cfg, None, theta)


def _acts(cfg, core, B):
    """-> {camera: [ReLU output of layer 0..3]} of the last encoder pass, over B images per camera"""
    out = {k: [] for k in cfg.image_keys}
    for l, (h, w) in enumerate(SC.out_dims(cfg.H, cfg.W)):
        c = SC.FEAT[l + 1]
        a = core.debug(f"small_act{l}", cfg.n_cam * B * h * w * c).reshape(cfg.n_cam, B, h, w, c)
        for i, k in enumerate(cfg.image_keys):
            out[k].append(a[i])
    return out


def _conv_grads(cfg, core):
    """-> {conv leaf (oracle name): gradient as the last critic phase left it}"""
    sl, _ = AH.leaf_slices(cfg)
    g = core.debug("g_critic", sl["enc/proprio/ln/bias"][1]).astype(np.float64)
    return {k: g[sl[k][0]:sl[k][1]] for k in SC.conv_leaves(cfg)}


def _measure(cfg, got_acts, got_grads, ref):
    """-> (forward error per (camera, layer), max-norm gradient error per conv leaf, element-wise gradient error per conv leaf)"""
    fwd = {(k, l): AH.rel_err(got_acts[k][l], ref["acts"][k][l]) for k in cfg.image_keys for l in range(SC.LAYERS)}
    gm, ge = {}, {}
    for k in SC.conv_leaves(cfg):
        r = ref["aux"]["grads"][k].numpy().reshape(-1)
        gm[k], ge[k] = AH.rel_err(got_grads[k], r), AH.elem_rel_err(got_grads[k], r, floor=1e-3)
    return fwd, gm, ge


def _update_critics_case(name, bounds=None, compare_state=True):
    """one update_critics of case `name` on the GPU against the fp64 oracle.  bounds: {"fwd" | "gm" | "ge": {key: bound}} in place
    of TOL / TOL / ELEM_TOL.  -> (core, the oracle's run, the activations read from the taps, the conv gradients)"""
    t0 = time.perf_counter()
    cfg, B, theta, b, noise = SC.inputs(name)
    ref = SC.reference(name)
    t1 = time.perf_counter()
    core = _make_core(name)
    core.update_critics(AH.batch_to_device(cfg, b), AH.noise_to_device(cfg, noise))
    got, info, aux = core.read_info(), ref["info"], ref["aux"]
    plan = [int(v) for v in core.debug("small_plan", 4)]
    acts, grads = _acts(cfg, core, B), _conv_grads(cfg, core)
    fwd, gm, ge = _measure(cfg, acts, grads, ref)
    print(f"{name}: small_plan {plan}; worst layer forward {max(fwd.values()):.2e}, worst conv gradient leaf {max(gm.values()):.2e}, "
          f"worst conv gradient element (>1e-3 of max) {max(ge.values()):.2e}; oracle {t1 - t0:.1f} s, GPU side {time.perf_counter() - t1:.1f} s")
    assert plan == SC.small_plan(cfg.H, cfg.W, B), plan
    if name in SC.BRANCH:
        assert plan == SC.BRANCH[name]["plan"], plan
    bounds = bounds or {}
    for key, e in fwd.items():
        assert e < bounds.get("fwd", {}).get(key, TOL), ("layer forward", key, e)
    for key, e in gm.items():
        assert e < bounds.get("gm", {}).get(key, TOL), ("conv gradient, max-norm", key, e)
    for key, e in ge.items():
        assert e < bounds.get("ge", {}).get(key, ELEM_TOL), ("conv gradient, element-wise", key, e)
    if not bounds:
        for k in ("critic_loss", "predicted_qs", "target_qs"):
            assert abs(got[k] - info[k]) < TOL * max(1.0, abs(info[k])), (k, got[k], info[k])
        q = core.debug("q", cfg.ensemble * B).reshape(cfg.ensemble, B)
        assert AH.rel_err(q, aux["q"].numpy()) < TOL
        assert AH.rel_err(core.debug("target_q", B), aux["target_q"].numpy()) < TOL
        x = core.debug("x", B * (cfg.enc_dim + cfg.A)).reshape(B, -1)
        assert AH.rel_err(x[:, :cfg.enc_dim], aux["enc_obs"].numpy()) < TOL
        _check_grads(cfg, core, aux["grads"], "g_critic", 0)
        if compare_state:
            _compare_state(cfg, ref["st"], core)
    assert core.step == ref["st"].step == 1
    return core, ref, acts, grads


# ------------------------------------------------------------------------------------------------------------------ branches
@pytest.mark.parametrize("name", list(SC.BRANCH))
def test_branch(gpu, name):
    _update_critics_case(name)


def test_four_cams_have_weights_of_their_own(gpu):
    """what four_cams rests on: the four cameras' conv stacks differ leaf by leaf, so a camera read at another's stride shows"""
    cfg, _, theta, _, _ = SC.inputs("four_cams")
    for l in range(SC.LAYERS):
        ws = [theta[f"enc/{k}/conv{l}/kernel"] for k in cfg.image_keys]
        assert all(not np.array_equal(ws[i], ws[j]) for i in range(4) for j in range(i))


def test_two_shards(gpu):
    """2 cameras, 33x47, B = 6 as two set_shard halves through begin_update / encode / critic_grads: the conv-gradient leaves of
    the halves, summed, are the full batch's, at the figure of tests/test_agent_gpu.py::test_dp_split_equals_full_batch"""
    cfg, B, theta, b, noise = SC.inputs("two_shards")

    def rows(tree, lo, hi):
        return {k: ({c: m[lo:hi] for c, m in v.items()} if isinstance(v, dict) else (v if k == "redq_idx" else v[lo:hi])) for k, v in tree.items()}

    def run(n, shard):
        core = AH.load_leaves(AH.make_core(cfg, n), cfg, None, theta)
        lo = 0 if shard is None else shard * n
        if shard is not None:
            core.set_shard(lo, B)
        # (the SmallEncoder reads the frames inside critic_grads: the batch has to outlive encode)
        db, dn = AH.batch_to_device(cfg, rows(b, lo, lo + n)), AH.noise_to_device(cfg, rows(noise, lo, lo + n))
        core.begin_update()
        core.encode(db)
        core.critic_grads(0, n, B, dn)
        return _conv_grads(cfg, core)
    full, parts = run(B, None), [run(B // 2, r) for r in range(2)]
    worst = 0.0
    for k in SC.conv_leaves(cfg):
        e = AH.rel_err(parts[0][k] + parts[1][k], full[k])
        worst = max(worst, e)
        assert np.abs(full[k]).max() > 0 and e < 1e-5, (k, e)
    print(f"two_shards: worst conv gradient leaf, two halves against the full batch: {worst:.2e}")


def test_a_fifth_camera_is_refused_at_creation(gpu):
    from serl_amd._lib import SerlError
    cfg = O.Config(image_keys=SC.CAMS4 + ("fifth",), H=32, W=32, S=SC.S_DIM, A=SC.A_DIM, encoder_type="small")
    with pytest.raises(SerlError, match=r"n_cam 5 not in \[0,4\]"):
        AH.make_core(cfg, 2)


# ------------------------------------------------------------------------------------------------------------------ regimes
def test_dead_channels(gpu):
    """channels 0 and cout - 1 of every layer have bias -1e3: exact zeros on the GPU in those channels of every layer's output, in
    their kernel column and bias entry of the gradient, and in the next layer's kernel rows that read them; the rest against fp64"""
    core, ref, acts, grads = _update_critics_case("dead_channels")
    cfg = SC.config("dead_channels")
    for k in cfg.image_keys:
        for l in range(SC.LAYERS):
            dead = list(SC.dead_of(l))
            assert (acts[k][l][..., dead] == 0).all(), (k, l)
            gk = grads[f"enc/{k}/conv{l}/kernel"].reshape(3, 3, SC.FEAT[l], SC.FEAT[l + 1])
            assert (gk[..., dead] == 0).all() and (grads[f"enc/{k}/conv{l}/bias"][dead] == 0).all(), (k, l)
            if l > 0:
                assert (gk[:, :, list(SC.dead_of(l - 1)), :] == 0).all(), (k, l)
            assert np.abs(gk).max() > 0


def test_flat_frames(gpu):
    """zero biases; image 0 all 0 (every pre-activation exactly 0: the `> 0` masks at equality, where the oracle's relu has
    gradient 0), image 1 all 255, a 0 / 255 step, a one-pixel checkerboard (the byte -> float table at its ends)"""
    core, ref, acts, grads = _update_critics_case("flat_frames")
    cfg = SC.config("flat_frames")
    for k in cfg.image_keys:
        for l in range(SC.LAYERS):
            assert (acts[k][l][0] == 0).all() and (acts[k][l][1] > 0).any(), (k, l)


def test_trained_scale(gpu):
    """conv kernels x 4 per layer, biases from [-0.5, 0.5], 33x47: layer-3 activations in the hundreds, where a lost piece of the
    bf16 x 3 split of the implicit GEMMs would show.  Judged against the fp64 oracle with the float32 oracle as yardstick, as
    tests/trained_regime.py: a figure's bound is TOL (ELEM_TOL element-wise) wherever the float32 oracle itself meets it, 4 x the
    float32 oracle's own figure otherwise.  Measured: the float32 oracle meets TOL and ELEM_TOL in every figure (worst layer forward
    see the printed line), so no bound is widened."""
    name = "trained_scale"
    cfg, B, _, _, _ = SC.inputs(name)
    ref, r32 = SC.reference(name), SC.reference(name, torch.float32)
    g32 = {k: r32["aux"]["grads"][k].numpy().reshape(-1).astype(np.float64) for k in SC.conv_leaves(cfg)}
    fwd32, gm32, ge32 = _measure(cfg, r32["acts"], g32, ref)
    print(f"{name}: float32 oracle against fp64: worst layer forward {max(fwd32.values()):.2e}, worst conv gradient leaf "
          f"{max(gm32.values()):.2e}, worst conv gradient element {max(ge32.values()):.2e}")
    bounds = {"fwd": {k: TOL if e < TOL else 4 * e for k, e in fwd32.items()},
              "gm": {k: TOL if e < TOL else 4 * e for k, e in gm32.items()},
              "ge": {k: ELEM_TOL if e < ELEM_TOL else 4 * e for k, e in ge32.items()}}
    core, ref, acts, grads = _update_critics_case(name, bounds)
    assert max(float(a.max()) for k in cfg.image_keys for a in acts[k][3:]) >= 100.0
    # the rest of the update under the same rule: the figure of the float32 oracle decides each bound
    got, info, i32 = core.read_info(), ref["info"], r32["info"]
    for k in ("critic_loss", "predicted_qs", "target_qs"):
        e32 = abs(i32[k] - info[k]) / max(1.0, abs(info[k]))
        assert abs(got[k] - info[k]) / max(1.0, abs(info[k])) < (TOL if e32 < TOL else 4 * e32), (k, got[k], info[k], e32)
    x = core.debug("x", B * (cfg.enc_dim + cfg.A)).reshape(B, -1)
    e32 = AH.rel_err(r32["aux"]["enc_obs"].numpy(), ref["aux"]["enc_obs"].numpy())
    assert AH.rel_err(x[:, :cfg.enc_dim], ref["aux"]["enc_obs"].numpy()) < (TOL if e32 < TOL else 4 * e32)


def test_high_utd(gpu):
    """update_high_utd(2) on dead_channels' parameters, B = 6: the second minibatch starts at image 3 of the frames"""
    name = "high_utd"
    cfg, B, theta, b, noise = SC.inputs(name)
    t0 = time.perf_counter()
    ref = SC.reference(name)
    core = _make_core(name)
    core.update_high_utd(AH.batch_to_device(cfg, b), 2, AH.noise_to_device(cfg, noise))
    got = core.read_info()
    for k, v in ref["info"].items():
        assert abs(got[k] - v) < TOL * max(1.0, abs(v)), (k, got[k], v)
    sl, _ = AH.leaf_slices(cfg)
    _check_grads(cfg, core, ref["aux"]["g_actor"], "g_actor", sl["enc/proprio/dense/kernel"][0])
    worst = _compare_state(cfg, ref["st"], core, steps=3)
    assert core.step == ref["st"].step == 3
    print(f"{name}: worst parameter leaf (99.9th percentile) {worst:.2e}; {time.perf_counter() - t0:.1f} s")
