"""What tests/test_small_encoder_branches_gpu.py rests on, checked without a GPU (tests/small_encoder_cases.py):
  * the plan arithmetic restated in Python gives every number the case table states, so a silent change of a constant shows;
  * the fp64 statement layer by layer, composed, is the oracle's encoder output bit for bit;
  * the regime inputs meet their conditions on the fp64 oracle: dead channels are dead, the all-zero image stays all-zero through
    the four layers, and every relu pre-activation of trained_scale keeps its margin with no element left out."""
import numpy as np
import pytest
import torch

from oracle import drq_oracle as O
import agent_helpers as AH
import small_encoder_cases as SC


@pytest.mark.parametrize("name", sorted(SC.BRANCH))
def test_plan_arithmetic_reproduces_the_case_table(name):
    c = SC.BRANCH[name]
    c0, sp = SC.plan(c["H"], c["W"], c["B"])
    assert SC.small_plan(c["H"], c["W"], c["B"]) == c["plan"]
    assert (c0["rows"], c0["chunks"], c0["per"], c0["empty"]) == (c["rows0"], c["plan"][0], c["per"], c["empty"])
    assert c0["nonempty"] == c.get("nonempty", c["plan"][0]) and 0 < c0["last"] <= c0["per"]
    assert (c0["nonempty"] - 1) * c0["per"] + c0["last"] == c0["rows"]
    if "rows" in c:
        assert [s["rows"] for s in sp] == c["rows"] and [s["kper"] for s in sp] == c["kper"]
    for s in sp:        # every slice of a K-split holds rows
        assert 0 < s["last"] <= s["kper"] and (s["S"] - 1) * s["kper"] + s["last"] == s["rows"]
    if "last1" in c:
        assert sp[0]["last"] == c["last1"]


def test_plan_figures_the_issue_states():
    """the figures written out once more, by hand, against the functions"""
    assert SC.conv0_plan(225) == {"chunks": 1, "per": 232, "nonempty": 1, "empty": 0, "last": 225}
    assert SC.conv0_plan(675) == {"chunks": 2, "per": 344, "nonempty": 2, "empty": 0, "last": 331}
    assert SC.conv0_plan(262353) == {"chunks": 1024, "per": 264, "nonempty": 994, "empty": 30, "last": 201}
    assert SC.conv0_plan(560263) == {"chunks": 1024, "per": 552, "nonempty": 1015, "empty": 9, "last": 535}
    assert SC.split_plan(131175) == {"S": 64, "kper": 2080, "last": 135}
    assert SC.split_plan(61425) == {"S": 29, "kper": 2144, "last": 1393}
    assert SC.split_plan(5247) == {"S": 2, "kper": 2624, "last": 2623}
    # B = 583 is the smallest batch at 64x64 that reaches the cap of 64 slices
    assert SC.split_plan(SC.rows_cam(64, 64, 582, 1))["S"] == 63 and SC.split_plan(SC.rows_cam(64, 64, 583, 1))["S"] == 64
    # the bench shape (B = 256, 128x128) runs 64 / 28 / 6 slices and the chunk cap
    assert SC.small_plan(128, 128, 256) == [1024, 64, 28, 6]
    # 32x32 with one image: layer 3 is one row per camera (forward GEMM M = 1, weight-gradient GEMM K = 1, pool over one pixel)
    assert SC.out_dims(32, 32) == [(15, 15), (7, 7), (3, 3), (1, 1)] and SC.rows_cam(32, 32, 1, 3) == 1
    with open(__file__.replace("tests/test_small_encoder_cases_cpu.py", "serl_amd/csrc/small_encoder.hip")) as f:
        src = " ".join(f.read().split())
    assert "constexpr int kConv0Chunks = 1024, kSmallMaxCams = 4;" in src
    assert "std::min<long>(kConv0Chunks, std::max<long>(1, rows_cam / 256))" in src
    assert "std::min<long>(64, std::max<long>(1, rows_cam / 2048))" in src


@pytest.mark.parametrize("name", ["four_cams", "trained_scale"])
def test_layers_composed_are_the_oracles_encoder_bit_for_bit(name):
    cfg, B, theta, b, _ = SC.inputs(name)
    th = O.to_torch(theta, torch.float64)
    dims = SC.out_dims(cfg.H, cfg.W)
    for k in cfg.image_keys:
        img = torch.tensor(b["obs"][k])
        pre, act, pooled = SC.layers_of(th, k, img)
        assert [tuple(a.shape) for a in act] == [(B, h, w, SC.FEAT[l + 1]) for l, (h, w) in enumerate(dims)]
        assert torch.equal(pooled, O.small_encoder_trunk(th, k, img)) and torch.equal(pooled, act[3].mean(dim=(1, 2)))
        x = img.to(torch.float64) / 255.0
        for l in range(SC.LAYERS):      # each layer from the one below: the tensors handed out are the ones the encoder computed
            p = O.conv_nhwc(x, th[f"enc/{k}/conv{l}/kernel"], 2, ((0, 0), (0, 0))) + th[f"enc/{k}/conv{l}/bias"]
            assert torch.equal(p, pre[l]) and torch.equal(torch.relu(p), act[l])
            x = act[l]
    # and through encode(): the encoder output of the update is built on this pooled vector
    enc = O.encode(th, cfg, {k: torch.tensor(v) for k, v in b["obs"].items()}, torch.tensor(b["state"], dtype=torch.float64))
    assert torch.equal(enc, SC.reference(name)["aux"]["enc_obs"])


def test_dead_channels_are_dead():
    cfg, B, theta, b, _ = SC.inputs("dead_channels")
    r = SC.reference("dead_channels")
    for k in cfg.image_keys:
        for l in range(SC.LAYERS):
            dead = list(SC.dead_of(l))
            live = [c for c in range(SC.FEAT[l + 1]) if c not in dead]
            act = r["acts"][k][l]
            fires = (act[..., live] > 0).any(axis=(0, 1, 2))      # (white noise leaves some channels of the deeper layers silent too)
            assert (act[..., dead] == 0).all() and fires.mean() > 0.5, (k, l)
            gk, gb = r["aux"]["grads"][f"enc/{k}/conv{l}/kernel"].numpy(), r["aux"]["grads"][f"enc/{k}/conv{l}/bias"].numpy()
            assert (gk[..., dead] == 0).all() and (gb[dead] == 0).all() and (gb[live][fires] != 0).all(), (k, l)
            if l > 0:       # the rows of this layer's kernel that read the dead channels of the layer below
                below = list(SC.dead_of(l - 1))
                assert (gk[:, :, below, :] == 0).all(), (k, l)
    r32 = SC.reference("dead_channels", torch.float32)       # float32 takes every relu of the differentiated pass to the same side
    for k in cfg.image_keys:
        for l in range(SC.LAYERS):
            assert np.array_equal(r32["acts"][k][l] > 0, r["acts"][k][l] > 0), (k, l)
            live = [c for c in range(SC.FEAT[l + 1]) if c not in SC.dead_of(l)]
            pre = SC.layers_of(O.to_torch(theta, torch.float64), k, torch.tensor(b["obs"][k]))[0][l][..., live]
            assert float(pre.abs().min() / pre.abs().max()) >= SC.FLIP_MARGIN, (k, l)
            assert (theta[f"enc/{k}/conv{l}/bias"][list(SC.dead_of(l))] == SC.DEAD_BIAS).all()
    hi = SC.inputs("high_utd")
    assert all(np.array_equal(theta[n], hi[2][n]) for n in theta) and hi[1] == 6 and SC.CASES["high_utd"]["utd"] == 2


def test_flat_frames_image_0_is_zero_through_all_layers():
    cfg, B, theta, b, _ = SC.inputs("flat_frames")
    th = O.to_torch(theta, torch.float64)
    for side in ("obs", "next"):
        for k in cfg.image_keys:
            f = b[side][k]
            assert (f[0] == 0).all() and (f[1] == 255).all() and set(np.unique(f[2])) == {0, 255} and (f[2][:, 0] == 0).all()
            assert (f[2][:, -1] == 255).all() and (f[3][::2, ::2] == 0).all() and (f[3][::2, 1::2] == 255).all()
            assert len(np.unique(f[4])) > 100
            pre, act, pooled = SC.layers_of(th, k, torch.tensor(f))
            for l in range(SC.LAYERS):
                assert (th[f"enc/{k}/conv{l}/bias"] == 0).all()
                assert (pre[l][0] == 0).all() and (act[l][0] == 0).all() and (act[l][1] > 0).any(), (side, k, l)
            assert (pooled[0] == 0).all()
    # relu's gradient at 0 is 0 in the oracle (torch, as jax.nn.relu): image 0 contributes nothing to a conv gradient
    x = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    torch.relu(x).sum().backward()
    assert (x.grad == 0).all()


@pytest.mark.parametrize("name", sorted(SC.BRANCH))
def test_branch_cases_decide_every_relu_as_float32_does(name):
    """the pass a branch case differentiates keeps FLIP_MARGIN with nothing excluded, float32 stays within half of it of fp64 in every
    layer and takes every relu to the same side: what the 1e-4 of the GPU test rests on at 560 000 rows"""
    cfg = SC.config(name)
    r, r32 = SC.reference(name), SC.reference(name, torch.float32)
    print(f"{name}: smallest |pre-activation| / layer max of the differentiated pass = {r['obs_margin']:.3e}")
    assert r["obs_margin"] >= SC.FLIP_MARGIN
    worst = 0.0
    for k in cfg.image_keys:
        for l in range(SC.LAYERS):
            assert np.array_equal(r32["acts"][k][l] > 0, r["acts"][k][l] > 0), (k, l)
            worst = max(worst, AH.rel_err(r32["acts"][k][l], r["acts"][k][l]))
    g = max(AH.rel_err(r32["aux"]["grads"][k].numpy(), r["aux"]["grads"][k].numpy()) for k in SC.conv_leaves(cfg))
    print(f"{name}: float32 oracle against fp64: worst layer forward {worst:.2e}, worst conv gradient leaf {g:.2e}")
    assert worst <= SC.FLIP_MARGIN / 2 and g < 2e-5


def test_trained_scale_keeps_the_relu_margin_with_nothing_excluded():
    cfg, B, theta, b, _ = SC.inputs("trained_scale")
    _, init = O.init_params(cfg, SC.PARAM_SEED)
    for k in cfg.image_keys:
        for l in range(SC.LAYERS):
            assert np.array_equal(theta[f"enc/{k}/conv{l}/kernel"], init[f"enc/{k}/conv{l}/kernel"] * np.float32(SC.KERNEL_SCALE))
            bias = theta[f"enc/{k}/conv{l}/bias"]
            assert np.abs(bias).max() <= SC.BIAS_RANGE and np.abs(bias).max() > 0.4 and len(np.unique(bias)) == bias.size
    r = SC.reference("trained_scale")
    # every pre-activation of every conv layer of every encoder pass of the update (policy and target critic at the next
    # observations, critic at the observations), both cameras: 3 passes x 2 cameras x B images
    per_image = sum(h * w * SC.FEAT[l + 1] for l, (h, w) in enumerate(SC.out_dims(cfg.H, cfg.W)))
    assert r["margin"].seen == 3 * cfg.n_cam * B * per_image
    print(f"trained_scale: smallest |pre-activation| / layer max = {r['margin'].worst:.3e} over {r['margin'].seen} pre-activations")
    assert r["margin"].worst >= SC.RELU_MARGIN
    top = max(float(a.max()) for a in (r["acts"][k][3] for k in cfg.image_keys))
    print(f"trained_scale: largest layer-3 activation {top:.1f}")
    assert top >= 100.0                    # "layer-3 activations reach the hundreds"
    # the float32 oracle is a usable yardstick here: its relu masks are the fp64 oracle's
    r32 = SC.reference("trained_scale", torch.float32)
    for k in cfg.image_keys:
        for l in range(SC.LAYERS):
            assert np.array_equal(r32["acts"][k][l] > 0, r["acts"][k][l] > 0), (k, l)
