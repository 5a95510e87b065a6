"""CPU side of the shape-edge parity tests: what the size table of tests/shape_edges.py covers, derived in plain Python, and
the oracle's and the jax stand-in's own padding at odd extents against PyTorch with the pads written out by hand."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import drq_oracle as O
import shape_edges as SE

D = torch.float64


def _shim():
    """the flax.linen stand-in the goldens were recorded under (it imports its sibling `jax` stand-in by that name)"""
    p = os.path.join(os.path.dirname(os.path.abspath(O.__file__)), "jaxshim")
    if p not in sys.path:
        sys.path.insert(0, p)
    import flax.linen as nn
    return nn


def _classes(H, W):
    """Rows and columns are separate classes wherever a kernel computes them in separate expressions (pads, window starts)."""
    gh, gw = SE.geometry(H, W)
    c = set()
    for axis, g in (("rows", gh), ("columns", gw)):
        c.add("conv_init reads %d high pad lines, %s" % (g["conv_init_pad_read"][1], axis))
        c.add("pool pad lo %d, %s" % (g["pool_pad"][0], axis))
        for i in (1, 2, 3):
            c.add("stage %d stride-2 pad %s, %s" % (i, g["conv0_pad"][i], axis))
    for i in (1, 2, 3):
        lo_h, lo_w = gh["conv0_pad"][i][0], gw["conv0_pad"][i][0]
        if lo_h != lo_w:
            c.add("pad %d, padw %d" % (lo_h, lo_w))
    h0, w0 = gh["conv_init_out"], gw["conv_init_out"]
    if h0 % 16 or w0 % 16:
        c.add("separate pooling")
    elif gw["pool_out"] not in (32, 16):
        c.add("fused pooling without the row-slab kernels")
    hw = SE.feat_hw(H, W)
    if hw not in (4, 8, 16):
        c.add("HW=%d" % hw)
    if hw >= 36:
        c.add("HW>=36")
    if min(H, W) == 32:
        c.add("an extent at the minimum")
    if H % 2 and W % 2 and max(H, W) < 48:
        c.add("both extents odd, below 48")
    return c


def test_the_size_table_covers_every_class():
    have = set()
    for H, W in SE.SIZES:
        have |= _classes(H, W)
    need = {"pad 1, padw 0", "pad 0, padw 1", "separate pooling", "fused pooling without the row-slab kernels",
            "HW=9", "HW=12", "HW>=36", "an extent at the minimum", "both extents odd, below 48"}
    for axis in ("rows", "columns"):
        # conv_init's explicit (3, 3): all three bottom / right pad lines are read at an odd extent, two at an even one
        need |= {f"conv_init reads 3 high pad lines, {axis}", f"conv_init reads 2 high pad lines, {axis}",
                 f"pool pad lo 1, {axis}", f"pool pad lo 0, {axis}"}
        for i in (1, 2, 3):
            need |= {f"stage {i} stride-2 pad (1, 1), {axis}", f"stage {i} stride-2 pad (0, 1), {axis}"}
    assert need <= have, sorted(need - have)


def test_the_geometry_is_the_oracles():
    """shape_edges.geometry against the extents the fp64 oracle actually produces (zero weights: shapes only)."""
    tp = {k: torch.zeros(s, dtype=torch.float32) for k, s in O.trunk_param_shapes().items()}
    for H, W in SE.SIZES:
        if H * W > 112 * 112:
            continue
        _, inter = O.trunk_forward(tp, torch.zeros((1, H, W, 3), dtype=torch.uint8), torch.float32, return_intermediates=True)
        gh, gw = SE.geometry(H, W)
        assert inter["conv_init"].shape[1:3] == (gh["conv_init_out"], gw["conv_init_out"])
        assert inter["pool"].shape[1:3] == (gh["pool_out"], gw["pool_out"])
        for i in range(4):
            assert inter[f"b{i}_out"].shape[1:3] == (gh["stage_out"][i], gw["stage_out"][i]), (H, W, i)
        assert SE.feat_hw(H, W) == O.Config(image_keys=("a",), H=H, W=W).feat_hw[0] * O.Config(image_keys=("a",), H=H, W=W).feat_hw[1]


def test_update_cases_are_the_edges_they_claim():
    ids = [c[0] for c in SE.UPDATE_CASES]
    assert len(set(ids)) == len(ids)
    seen = set()
    for case in SE.UPDATE_CASES:
        cfg, B, utd = SE.update_config(case)
        assert B % utd == 0
        seen.add(("A", cfg.A)), seen.add(("ncam", cfg.n_cam)), seen.add(("E", cfg.ensemble)), seen.add(("sub", cfg.subsample))
        if cfg.image_keys and not cfg.small:
            seen.add(("HW", SE.feat_hw(cfg.H, cfg.W)))
        if (B * cfg.ensemble) % 64:
            seen.add("M tail")
        if cfg.S % 16 or (cfg.S + 64) % 16:
            seen.add("K tail")
        if cfg.backup_entropy:
            seen.add("backup_entropy")
    assert {("A", 1), ("A", 64), ("A", 33), ("ncam", 0), ("ncam", 3), ("ncam", 4), ("E", 17), ("E", 16), ("E", 2), ("sub", None), ("sub", 1),
            ("HW", 4), ("HW", 9), ("HW", 12), ("HW", 49), "M tail", "K tail", "backup_entropy"} <= seen


# ---- padding at odd extents: pads written out by hand, PyTorch does the rest --------------------------------------------------
# n, k, s -> (lo, hi) by XLA's rule, worked out on paper: out = ceil(n / s), total = (out - 1) * s + k - n
HAND_PADS = [((47, 7, 2), (3, 3)),     # out 24: 46 + 7 - 47 = 6
             ((33, 7, 2), (3, 3)),     # out 17: 32 + 7 - 33 = 6
             ((84, 7, 2), (2, 3)),     # out 42: 82 + 7 - 84 = 5
             ((17, 3, 2), (1, 1)),     # out 9: 16 + 3 - 17 = 2
             ((21, 3, 2), (1, 1)),     # out 11: 20 + 3 - 21 = 2
             ((42, 3, 2), (0, 1)),     # out 21: 40 + 3 - 42 = 1
             ((9, 3, 1), (1, 1)),
             ((5, 1, 2), (0, 0)), ((6, 1, 2), (0, 0))]


@pytest.mark.parametrize("nks,expect", HAND_PADS)
def test_same_pad_at_odd_extents(nks, expect):
    assert O.same_pad(*nks) == expect
    assert _shim()._same_pads(*nks) == expect


@pytest.mark.parametrize("H,W", [(33, 47), (17, 24), (21, 21), (9, 12)])
def test_max_pool_same_at_odd_extents_against_a_hand_padded_tensor(H, W):
    """3x3 stride-2 SAME max-pool: an odd extent has ONE -inf line on each side, an even one only below / right.  The stand-in's
    nn.max_pool against F.max_pool2d on a tensor padded by hand (the oracle's own pooling lines: the next test)."""
    nn = _shim()
    x = torch.randn(2, H, W, 5, dtype=D) - 3.0            # mostly negative: a zero pad (instead of -inf) would win the maximum
    pt, pb = (1, 1) if H % 2 else (0, 1)
    pl, pr = (1, 1) if W % 2 else (0, 1)
    xp = torch.full((2, 5, H + pt + pb, W + pl + pr), float("-inf"), dtype=D)
    xp[:, :, pt:pt + H, pl:pl + W] = x.permute(0, 3, 1, 2)
    ref = F.max_pool2d(xp, 3, 2).permute(0, 2, 3, 1)
    assert ref.shape[1:3] == (SE.cdiv(H, 2), SE.cdiv(W, 2)) and torch.isfinite(ref).all()
    got = torch.as_tensor(nn.max_pool(x, (3, 3), strides=(2, 2), padding="SAME"))
    assert got.shape == ref.shape and torch.equal(got, ref)
    assert (O.same_pad(H, 3, 2), O.same_pad(W, 3, 2)) == ((pt, pb), (pl, pr))
    # brute force, window by window: output (oy, ox) covers rows 2 oy - pt .. 2 oy - pt + 2 clipped to the map
    for oy in (0, ref.shape[1] - 1):
        for ox in (0, ref.shape[2] - 1):
            ys = [y for y in range(2 * oy - pt, 2 * oy - pt + 3) if 0 <= y < H]
            xs = [c for c in range(2 * ox - pl, 2 * ox - pl + 3) if 0 <= c < W]
            assert torch.equal(ref[:, oy, ox], x[:, ys][:, :, xs].amax(dim=(1, 2)))


@pytest.mark.parametrize("H,W", [(33, 47), (47, 33), (34, 34), (66, 40)])
def test_the_oracles_own_pooling_at_odd_extents_against_a_hand_padded_tensor(H, W):
    """O.trunk_forward's pooling lines themselves: its "pool" intermediate against F.max_pool2d on relu(GroupNorm(conv_init))
    padded by hand with -inf -- one line on each side of an odd extent, only below / right of an even one."""
    trunk, _ = O.init_params(O.Config(image_keys=("a",), H=H, W=W), 42)
    tp = O.to_torch(trunk, D)
    img = torch.randint(0, 256, (2, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(H * 100 + W))
    _, inter = O.trunk_forward(tp, img, D, return_intermediates=True)
    x = torch.relu(O.group_norm(inter["conv_init"], tp["trunk/norm_init/scale"], tp["trunk/norm_init/bias"]))
    h0, w0 = x.shape[1], x.shape[2]
    assert (h0, w0) == (SE.cdiv(H, 2), SE.cdiv(W, 2))
    pt, pl = h0 % 2, w0 % 2
    xp = torch.full((2, 64, h0 + pt + 1, w0 + pl + 1), float("-inf"), dtype=D)
    xp[:, :, pt:pt + h0, pl:pl + w0] = x.permute(0, 3, 1, 2)
    ref = F.max_pool2d(xp, 3, 2).permute(0, 2, 3, 1)
    assert inter["pool"].shape == ref.shape and torch.equal(inter["pool"], ref)
    if pt or pl:      # ... and the window start matters: without the low-side line the result is another tensor
        xq = torch.full((2, 64, h0 + 2, w0 + 2), float("-inf"), dtype=D)
        xq[:, :, :h0, :w0] = x.permute(0, 3, 1, 2)
        assert not torch.equal(F.max_pool2d(xq, 3, 2).permute(0, 2, 3, 1)[:, :ref.shape[1], :ref.shape[2]], ref)


@pytest.mark.parametrize("H,W", [(33, 47), (47, 33), (35, 84)])
def test_conv_init_shaped_conv_at_odd_extents_against_explicit_pads(H, W):
    """7x7 stride 2 on an odd extent: SAME is (3, 3), the same as the reference's explicit [(3, 3), (3, 3)]; on an even extent
    SAME is (2, 3) and differs from it.  Oracle conv_same / conv_nhwc and the stand-in's nn.Conv against F.conv2d with the pads
    written out."""
    nn = _shim()
    x = torch.randn(2, H, W, 3, dtype=D)
    w = torch.randn(7, 7, 3, 4, dtype=D)
    wt = w.permute(3, 2, 0, 1)

    def by_hand(pads_h, pads_w):
        return F.conv2d(F.pad(x.permute(0, 3, 1, 2), (pads_w[0], pads_w[1], pads_h[0], pads_h[1])), wt, stride=2).permute(0, 2, 3, 1)

    same_h, same_w = ((3, 3) if H % 2 else (2, 3)), ((3, 3) if W % 2 else (2, 3))
    ref_same, ref_explicit = by_hand(same_h, same_w), by_hand((3, 3), (3, 3))
    assert ref_same.shape == ref_explicit.shape == (2, SE.cdiv(H, 2), SE.cdiv(W, 2), 4)
    assert torch.allclose(O.conv_same(x, w, 2), ref_same, rtol=1e-12, atol=1e-12)
    assert torch.allclose(O.conv_nhwc(x, w, 2, ((3, 3), (3, 3))), ref_explicit, rtol=1e-12, atol=1e-12)
    if W % 2 == 0:
        assert not torch.allclose(ref_same, ref_explicit)       # the two conventions are different functions at an even extent

    class Net(nn.Module):
        padding: object = "SAME"

        @nn.compact
        def __call__(self, v):
            return nn.Conv(4, (7, 7), strides=(2, 2), padding=self.padding, use_bias=False, name="conv_init")(v)

    for padding, ref in (("SAME", ref_same), ([(3, 3), (3, 3)], ref_explicit)):
        got = Net(padding=padding).apply({"params": {"conv_init": {"kernel": w}}}, x)
        assert torch.allclose(torch.as_tensor(got), ref, rtol=1e-12, atol=1e-12), padding


@pytest.mark.parametrize("H,W", [(21, 25), (9, 12), (5, 6)])
def test_stride2_3x3_conv_at_odd_extents_against_explicit_pads(H, W):
    x = torch.randn(2, H, W, 6, dtype=D)
    w = torch.randn(3, 3, 6, 5, dtype=D)
    ph = (1, 1) if H % 2 else (0, 1)
    pw = (1, 1) if W % 2 else (0, 1)
    ref = F.conv2d(F.pad(x.permute(0, 3, 1, 2), (pw[0], pw[1], ph[0], ph[1])), w.permute(3, 2, 0, 1), stride=2).permute(0, 2, 3, 1)
    assert torch.allclose(O.conv_same(x, w, 2), ref, rtol=1e-12, atol=1e-12)
