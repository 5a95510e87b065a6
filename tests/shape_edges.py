"""Image sizes and update-chain dimensions off the powers of two, shared by test_shape_edges_cpu.py (which proves what the
table covers) and test_shape_edges_gpu.py (which runs it on the HIP path).

The frozen trunk (resnet_v1.py:189-286) halves the extent five times, rounding up: conv_init 7x7/2 with the EXPLICIT padding
[(3, 3), (3, 3)] (resnet_v1.py:249-255 -- not "SAME": an even extent leaves the third bottom / right pad line unread, an odd
one reads all three), max_pool 3x3/2 "SAME" (:259), then the four ResNetBlocks with strides 1, 2, 2, 2 whose 3x3 convs are
"SAME" (:143-156).  XLA's SAME puts total // 2 on the low side: a stride-2 3x3 window over an even extent is padded (0, 1),
over an odd one (1, 1); the -inf row above the image in the max-pool exists only for an odd pooled extent."""
from oracle import drq_oracle as O

# (H, W).  test_shape_edges_cpu.py::test_the_size_table_covers_every_class fails if an edit drops a class.
# (33, 47) has the odd pooled extent and the (1, 1) stride-2 pads along the rows, (47, 33) the same along the columns: the kernels
# treat the two axes in separate expressions.
SIZES = [(84, 84), (96, 96), (100, 80), (72, 112), (33, 47), (47, 33), (32, 32), (224, 224)]


def cdiv(a, b):
    return -(-a // b)


def axis_geometry(n):
    """One image axis of extent n -> dict of the extents and low/high pads the trunk meets along it."""
    h0 = (n + 2 * 3 - 7) // 2 + 1                      # conv_init, explicit pad 3
    assert h0 == cdiv(n, 2)
    read_hi = (h0 - 1) * 2 + 7 - 3 - n                 # pad lines below / right of the image that a window reaches
    h1 = cdiv(h0, 2)
    ext = [h1]                                         # input extent of stage 0, then the output of every stage
    pads = []                                          # (lo, hi) of conv0 of stage i
    for _, s in O.STAGES:
        pads.append(O.same_pad(ext[-1], 3, s))
        ext.append(cdiv(ext[-1], s))
    return {"conv_init_out": h0, "conv_init_pad_read": (3, read_hi), "pool_pad": O.same_pad(h0, 3, 2), "pool_out": h1,
            "stage_in": ext[:-1], "stage_out": ext[1:], "conv0_pad": pads}


def geometry(H, W):
    return axis_geometry(H), axis_geometry(W)


def feat_hw(H, W):
    gh, gw = geometry(H, W)
    return gh["stage_out"][-1] * gw["stage_out"][-1]


def expected_pads(H, W):
    """{plan layer name: (low pad of the rows, of the columns)} as XLA's SAME gives them (O.same_pad)."""
    gh, gw = geometry(H, W)
    out = {}
    for i, (_, s) in enumerate(O.STAGES):
        out[f"b{i}_conv0"] = (gh["conv0_pad"][i][0], gw["conv0_pad"][i][0])
        out[f"b{i}_conv1"] = (1, 1)
        if i > 0:
            out[f"b{i}_proj"] = (0, 0)                 # 1x1: never padded
    return out


# Update-chain rows: (id, image_keys, encoder, H, W, S, A, ensemble, subsample, B, utd of the high-UTD leg, backup_entropy)
UPDATE_CASES = [
    ("3cam_33x47_all_ones", ("a", "b", "c"), "resnet-pretrained", 33, 47, 1, 1, 3, 2, 1, 1, False),
    ("1cam_84_A64_E17_B65", ("wrist",), "resnet-pretrained", 84, 84, 65, 64, 17, 2, 65, 5, False),
    ("4cam_100x80_A33_B7", ("a", "b", "c", "d"), "resnet-pretrained", 100, 80, 17, 33, 2, 2, 7, 7, True),
    ("state_S130_E16_B129", (), None, 0, 0, 130, 8, 16, None, 129, 3, False),
    ("state_S3_A64_B63", (), None, 0, 0, 3, 64, 2, 1, 63, 3, False),
    ("state_S3_A64_B64", (), None, 0, 0, 3, 64, 2, 1, 64, 4, False),
    ("small_72x112_B5", ("front", "wrist"), "small", 72, 112, 5, 3, 10, 2, 5, 5, False),
    ("small_84_B6", ("front", "wrist"), "small", 84, 84, 5, 3, 10, 2, 6, 2, False),
    ("small_33x47_B6", ("front", "wrist"), "small", 33, 47, 5, 3, 10, 2, 6, 3, False),
    ("2cam_224_B4", ("front", "wrist"), "resnet-pretrained", 224, 224, 24, 6, 10, 2, 4, 2, False),
]


def update_config(case):
    _, keys, enc, H, W, S, A, E, sub, B, utd, bent = case
    kw = dict(image_keys=keys, S=S, A=A, ensemble=E, subsample=sub, backup_entropy=bent)
    if keys:
        kw.update(H=H, W=W, encoder_type=enc)
    else:
        kw.update(discount=0.99)
    return O.Config(**kw), B, utd
