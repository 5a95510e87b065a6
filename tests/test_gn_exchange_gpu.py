"""The statistics exchange of the fused GroupNorm epilogues (serl_amd/csrc/trunk_f16x3_common.h: LOCAL epilogues where a tile is a
whole image, data-tagged granule records where an image is spread over 2..4 row tiles; bookkeeping in gn_exchange.h, proved on the
CPU in test_gn_exchange_cpu.py).  Bounds are the suite's: 2e-6 of max-abs between the fused pass and the pass with separate
GroupNorm passes (SERL_GN_FUSE=0), 5e-6 of the fp64 oracle on the first and last six images (GroupNorm is per image, so those
images are checked completely) -- tests/test_agent_gpu.py::test_row_slab_kernels_fused_and_unfused."""
import pytest
import torch

from oracle import drq_oracle as O
import agent_helpers as AH

pytestmark = pytest.mark.gpu

# (frame rows, frame columns, images): what each shape runs is asserted from the library's own plan below
#   128 x 128, 128: records of G = 4 row tiles on both slab-DMA stage-0 convs, b1_conv0 on the 128 x 64 tile, b1_conv1 LOCAL
#   64 x 64, 128:   LOCAL on both stage-0 convs, split8 (mode 2) residual
#   64 x 64, 512:   the smallest raw-input shape: LOCAL in the raw-input kernel, mode-4 residual
#   128 x 64, 128:  G = 2
#   128 x 128, 512: raw input with G = 4, b1_conv0 on the 128 x 128 tile
SHAPES = [(128, 128, 128), (64, 64, 128), (64, 64, 512), (128, 64, 128), (128, 128, 512)]


def _assert_plan(plan, H, W, n):
    fused = {k: plan[k][3] for k in ("b0_conv0", "b0_conv1", "b1_conv0", "b1_conv1") if k in plan}
    assert plan["b0_conv0"][0] == "S" and plan["b0_conv1"][:2] == ("S", 9), plan
    assert plan["raw_b0"] == (1 if n % 512 == 0 else 0), plan
    if (H, W) == (64, 64):
        assert fused["b0_conv0"] == 2 and fused["b0_conv1"] == 2, plan       # a 256 x 64 tile is the whole 16 x 16 map
    else:
        assert fused["b0_conv0"] == 1 and fused["b0_conv1"] == 1, plan       # 2 or 4 row tiles per image exchange records
    if (H, W) == (128, 128):
        assert plan["b1_conv1"][:2] == ("S", 9) and fused["b1_conv1"] == 2, plan
        assert plan["b1_conv0"][:2] == ("D", 4 if n == 128 else 0) and fused["b1_conv0"] == 1, plan


@pytest.mark.parametrize("H,W,n", SHAPES)
def test_fused_epilogues_match_the_separate_passes_and_the_oracle(gpu, H, W, n, monkeypatch):
    cfg = O.Config(image_keys=("a",), H=H, W=W, S=4, A=2)
    st, core = AH.make_pair(cfg, B=n // 2, trunk_mode="f16x3")
    img = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device="cuda", generator=torch.Generator("cuda").manual_seed(H + W + n))
    monkeypatch.setenv("SERL_GN_FUSE", "0")
    plain = core.trunk_forward(img).clone()
    assert core.trunk_plan()["b0_conv1"][3] == 0
    monkeypatch.delenv("SERL_GN_FUSE")
    scale = float(plain.abs().max())
    for rep in range(2):          # (the second pass runs on records that hold the first pass's granules)
        fused = core.trunk_forward(img).clone()
        plan = core.trunk_plan()
        _assert_plan(plan, H, W, n)
        d = float((fused - plain).abs().max()) / scale
        print(f"gn exchange {H}x{W} n={n} pass {rep}: fused vs separate {d:.2e}; plan {plan}")
        assert d < 2e-6, (rep, d)
    sel = list(range(6)) + list(range(n - 6, n))
    ref = O.trunk_forward(st.trunk, img[sel].cpu(), torch.float64).numpy()
    err = AH.rel_err(fused[sel].cpu().numpy(), ref)
    print(f"gn exchange {H}x{W} n={n}: rel err vs fp64 = {err:.2e}")
    assert err < 5e-6, err


def test_passes_are_bit_identical_under_uneven_load(gpu, monkeypatch):
    """The exchange sums an image's partials in a fixed order, so every pass over the same frames gives the same bits -- which a
    torn or stale granule would break.  20 passes of 128 images of 128 x 128 on one stream; on every other pass a second agent's
    update_high_utd (64 x 64 frames, B = 32: its own trunk passes, GEMMs, Adam) runs on another stream and competes for CUs and
    memory queues.  Only one fused pass may be in flight per process (the other falls back to the separate passes, whose bits
    differ), so the second agent runs with SERL_GN_FUSE=0 -- the switch is read per pass -- and every pass of the first is
    asserted to have been planned fused."""
    cfg = O.Config(image_keys=("a",), H=128, W=128, S=4, A=2)
    _, core = AH.make_pair(cfg, B=64, trunk_mode="f16x3")
    n = 128
    img = torch.randint(0, 256, (n, 128, 128, 3), dtype=torch.uint8, device="cuda", generator=torch.Generator("cuda").manual_seed(11))
    monkeypatch.setenv("SERL_GN_FUSE", "0")
    plain = core.trunk_forward(img).clone()
    scale = float(plain.abs().max())
    cfg2 = O.Config(image_keys=("front", "wrist"), H=64, W=64, S=5, A=3)
    _, core2 = AH.make_pair(cfg2, 32)
    db2 = AH.batch_to_device(cfg2, AH.synth_batch(cfg2, 32, seed=1))
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    first = None
    same = torch.ones((), dtype=torch.bool, device="cuda")
    worst = torch.zeros((), device="cuda")
    for it in range(20):
        monkeypatch.setenv("SERL_GN_FUSE", "1")
        with torch.cuda.stream(sa):
            got = core.trunk_forward(img)
            plan = core.trunk_plan()
            assert plan["b0_conv0"][3] == 1 and plan["b0_conv1"][3] == 1 and plan["b1_conv0"][3] == 1 and plan["b1_conv1"][3] == 2, (it, plan)
            if first is None:
                first = got.clone()
            same = same & (got == first).all()
            worst = torch.maximum(worst, (got - plain).abs().max())
        if it % 2 == 0:
            monkeypatch.setenv("SERL_GN_FUSE", "0")
            with torch.cuda.stream(sb):
                core2.update_high_utd(db2, 1, None)
    torch.cuda.synchronize()
    w = float(worst) / scale
    print(f"gn exchange under uneven load: 20 passes bit-identical {bool(same)}, worst vs separate passes {w:.2e}")
    assert bool(same)
    assert w < 2e-6, w
    assert all(v == v and abs(v) != float("inf") for v in core2.read_info().values())
