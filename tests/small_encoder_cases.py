"""Shared by tests/test_small_encoder_cases_cpu.py and tests/test_small_encoder_branches_gpu.py: the cases that take the trainable
SmallEncoder (serl_amd/csrc/small_encoder.hip) through every branch of its backward pass's launch plan and away from its
initialisation, the plan arithmetic restated, and the fp64 statement of the encoder layer by layer.

The launch plan depends on rows_cam = B * h * w of a layer's output, per camera:
  * layer 0's weight gradient: chunks = min(1024, max(1, rows_cam / 256)) workgroups per camera, each over
    per = roundup8(ceil(rows_cam / chunks)) rows; a chunk that starts past rows_cam writes zeros;
  * the weight-gradient GEMM of layers 1..3: a K-split over the rows, S = min(64, max(1, rows_cam / 2048)) slices of
    kper = roundup32(ceil(rows_cam / S)) rows (heads.hip's partition), halved while S * n_cam slabs exceed the workspace.
That halving needs S * n_cam > 64 on layer 3, about 65 000 layer-3 rows per camera with four cameras: no test-sized shape
reaches it, and no case here tries.

The fp64 statement is the oracle's own encoder (oracle.drq_oracle.small_encoder_trunk, which tests/test_reference_update.py pins
to the reference's SmallEncoder) with its per-layer tensors handed out; there is no second encoder here."""
import numpy as np
import torch

from oracle import drq_oracle as O
import agent_helpers as AH

FEAT = O.SMALL_FEATURES
LAYERS = 4
CHUNK_CAP, CHUNK_ROWS, SPLIT_CAP, SPLIT_ROWS = 1024, 256, 64, 2048     # kConv0Chunks, rows_cam / 256; the K-split's 64, rows_cam / 2048
RELU_MARGIN = 1e-4          # tests/mlp_plain.py's: distance of a relu pre-activation from 0, here relative to the layer's max
# Branch cases: a conv gradient is a sum over up to 560 000 rows, and ONE row whose relu falls on the other side in float32 than in
# fp64 moves a layer-0 leaf by 1e-4 of its largest entry (the float32 oracle itself: 8e-5 at chunk_cap with O.init_params' biases).
# So the pre-activations of the pass that is differentiated (the online encoder at the observations) keep this distance from 0,
# relative to the layer's largest: twice the worst forward error float32 may show there (measured 1.3e-6; the CPU test asserts 1.5e-6).
FLIP_MARGIN = 3e-6
S_DIM, A_DIM = 5, 3
PARAM_SEED, BATCH_SEED, NOISE_SEED = 42, 3, 7


# ---- plan arithmetic -------------------------------------------------------------------------------------------------------------
def out_dims(H, W):
    """-> [(h, w)] of the four layers' outputs: 3x3 kernels, stride 2, padding VALID"""
    out = []
    for _ in range(LAYERS):
        H, W = (H - 3) // 2 + 1, (W - 3) // 2 + 1
        out.append((H, W))
    return out


def rows_cam(H, W, B, layer):
    h, w = out_dims(H, W)[layer]
    return B * h * w


def _ceil(a, b):
    return -(-a // b)


def conv0_plan(rows):
    """layer 0's weight gradient over `rows` rows of one camera -> {"chunks", "per", "nonempty", "empty", "last"}: workgroups per
    camera, rows of a full chunk, chunks that hold rows, chunks that hold none, rows of the last chunk that holds any"""
    chunks = min(CHUNK_CAP, max(1, rows // CHUNK_ROWS))
    per = (_ceil(rows, chunks) + 7) // 8 * 8
    nonempty = min(chunks, _ceil(rows, per))
    return {"chunks": chunks, "per": per, "nonempty": nonempty, "empty": chunks - nonempty, "last": rows - (nonempty - 1) * per}


def split_plan(rows):
    """the K-split of a weight-gradient GEMM over `rows` rows of one camera -> {"S", "kper", "last"}: slices, rows of a full
    slice, rows of the last slice"""
    S = min(SPLIT_CAP, max(1, rows // SPLIT_ROWS))
    kper = (_ceil(rows, S) + 31) // 32 * 32
    return {"S": S, "kper": kper, "last": rows - (S - 1) * kper}


def plan(H, W, B):
    """-> ({"rows", **conv0_plan}, [{"rows", **split_plan} of layers 1, 2, 3]) of a pass over B images per camera"""
    r = [rows_cam(H, W, B, l) for l in range(LAYERS)]
    return dict(rows=r[0], **conv0_plan(r[0])), [dict(rows=r[l], **split_plan(r[l])) for l in (1, 2, 3)]


def small_plan(H, W, B):
    """what the debug tap small_plan reads after a backward pass at this shape: [chunks, S1, S2, S3]"""
    c0, sp = plan(H, W, B)
    return [c0["chunks"]] + [s["S"] for s in sp]


# ---- the case table ---------------------------------------------------------------------------------------------------------------
CAMS4 = ("front", "wrist", "side", "top")
# id -> keys, H, W, B and the plan numbers the issue states for it ("plan": the tap; the rest: what the Python arithmetic must give)
BRANCH = {
    "one_chunk": dict(keys=("wrist",), H=32, W=32, B=1, plan=[1, 1, 1, 1], rows0=225, per=232, empty=0),
    "two_chunks": dict(keys=("wrist",), H=32, W=32, B=3, plan=[2, 1, 1, 1], rows0=675, per=344, empty=0),
    "four_cams": dict(keys=CAMS4, H=33, W=47, B=3, plan=[4, 1, 1, 1], rows0=1104, per=280, empty=0),
    "chunk_cap": dict(keys=("front", "wrist"), H=64, W=64, B=273, plan=[1024, 29, 6, 1], rows0=262353, per=264, nonempty=994, empty=30,
                      rows=[61425, 13377, 2457], kper=[2144, 2240, 2464]),
    "split_cap": dict(keys=("wrist",), H=64, W=64, B=583, plan=[1024, 64, 13, 2], rows0=560263, per=552, nonempty=1015, empty=9,
                      rows=[131175, 28567, 5247], kper=[2080, 2208, 2624], last1=135),
}
REGIME = {
    "dead_channels": dict(keys=("front", "wrist"), H=64, W=64, B=6),
    "flat_frames": dict(keys=("front", "wrist"), H=64, W=64, B=6),
    "trained_scale": dict(keys=("front", "wrist"), H=33, W=47, B=6),
    "high_utd": dict(keys=("front", "wrist"), H=64, W=64, B=6, utd=2),       # dead_channels' parameters
    "two_shards": dict(keys=("front", "wrist"), H=33, W=47, B=6),
}
CASES = {**BRANCH, **REGIME}
DEAD_BIAS = -1e3
KERNEL_SCALE, BIAS_RANGE = 4.0, 0.5      # trained_scale: every conv kernel x 4, biases from [-0.5, 0.5]


def config(name):
    c = CASES[name]
    return O.Config(image_keys=c["keys"], H=c["H"], W=c["W"], S=S_DIM, A=A_DIM, encoder_type="small")


def conv_leaves(cfg):
    return [f"enc/{k}/conv{l}/{p}" for k in cfg.image_keys for l in range(LAYERS) for p in ("kernel", "bias")]


def dead_of(layer):
    """the channels dead_channels kills in a layer's output"""
    return (0, FEAT[layer + 1] - 1)


def _flat_images(b, cfg):
    """flat_frames: image 0 all 0, image 1 all 255, image 2 a vertical 0 / 255 step, image 3 a one-pixel checkerboard, in the
    observations and the next observations of every camera; the rest stay noise"""
    H, W = cfg.H, cfg.W
    step = np.zeros((H, W, 3), np.uint8)
    step[:, W // 2:] = 255
    yy, xx = np.mgrid[0:H, 0:W]
    checker = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    for side in ("obs", "next"):
        for k in cfg.image_keys:
            f = b[side][k]
            f[0], f[1], f[2], f[3] = 0, 255, step, checker
    return b


def _conv_pre(x, w):
    return O.conv_nhwc(x, w, 2, ((0, 0), (0, 0)))


def _clear_biases(cfg, theta, b, sides, margin, draw, kernel_scale=1.0, seed=17, dead=False):
    """-> theta with every conv kernel x kernel_scale and every conv bias drawn anew by draw(rng, n) (float candidates), channel by
    channel and layer by layer, a channel's bias being drawn again while a pre-activation of that channel -- any image of the
    batch's `sides` ("obs", "next") -- would lie within 1.25 x margin x the layer's largest of 0: the reseeding a relu comparison
    needs, done per channel (a layer 0 has 10^5 to 10^7 pre-activations per pass, and no seed of a whole recipe leaves all of them
    clear).  dead: channels dead_of(layer) get DEAD_BIAS instead, before the next layer is looked at.  What it built is asserted on the oracle's own run, nothing excluded, by tests/test_small_encoder_cases_cpu.py."""
    rng = np.random.default_rng(seed)
    out = {k: np.array(v, np.float32) for k, v in theta.items()}
    for k in cfg.image_keys:
        x = torch.cat([torch.tensor(b[s][k]) for s in sides]).to(torch.float64) / 255.0
        for l in range(LAYERS):
            w = out[f"enc/{k}/conv{l}/kernel"] = (out[f"enc/{k}/conv{l}/kernel"] * np.float32(kernel_scale)).astype(np.float32)
            with torch.no_grad():
                v = _conv_pre(x, torch.tensor(w, dtype=torch.float64))
            cout = FEAT[l + 1]
            vs = np.sort(v.reshape(-1, cout).numpy(), axis=0)                     # [positions][cout]
            reach = float(np.abs(draw(np.random.default_rng(0), 4096)).max())
            clear = 1.25 * margin * (np.abs(vs).max() + reach)                    # (the largest the layer can reach bounds its max)
            bias = np.zeros(cout, np.float32)
            for c in range(cout):
                col = np.ascontiguousarray(vs[:, c])
                cand = draw(rng, 4096).astype(np.float32)
                # where the draws find no clear spot (10^5 values of a channel and more), the middles of its widest clear gaps
                gaps = np.nonzero(np.diff(col) >= 2.5 * clear)[0]
                mid = -0.5 * (col[gaps] + col[gaps + 1])
                mid = mid[np.abs(mid) <= reach]
                cand = np.concatenate([cand, rng.permutation(mid).astype(np.float32)])
                at = -cand.astype(np.float64)
                i = np.searchsorted(col, at)
                near = np.minimum(np.abs(col[np.minimum(i, len(col) - 1)] - at), np.abs(col[np.maximum(i - 1, 0)] - at))
                good = np.nonzero(near >= clear)[0]
                assert len(good), f"no bias clears the relu margin: {k} layer {l} channel {c}"
                bias[c] = cand[good[0]]
            if dead:
                bias[list(dead_of(l))] = DEAD_BIAS
            out[f"enc/{k}/conv{l}/bias"] = bias
            x = torch.relu(v + torch.tensor(bias, dtype=torch.float64))
    return out


def _draw_trained(rng, n):
    return rng.uniform(-BIAS_RANGE, BIAS_RANGE, n)


def _draw_init(rng, n):
    return 0.1 * rng.standard_normal(n)          # O.init_params' jitter of a bias


_INPUTS = {}


def inputs(name):
    """-> (cfg, B, theta (oracle names, float32), batch, noise), numpy; memoised, read-only"""
    if name not in _INPUTS:
        c, cfg = CASES[name], config(name)
        B = c["B"]
        _, theta = O.init_params(cfg, PARAM_SEED)
        b = AH.synth_batch(cfg, B, seed=BATCH_SEED)
        noise = O.make_noise(cfg, B, seed=NOISE_SEED, utd_ratio=c.get("utd", 1))
        if name in ("dead_channels", "high_utd"):      # (the live channels keep FLIP_MARGIN like a branch case's)
            theta = _clear_biases(cfg, theta, b, ("obs",), FLIP_MARGIN, _draw_init, dead=True)
        elif name == "flat_frames":
            for k in cfg.image_keys:
                for l in range(LAYERS):
                    theta[f"enc/{k}/conv{l}/bias"][:] = 0.0
            _flat_images(b, cfg)
        elif name == "trained_scale":
            theta = _clear_biases(cfg, theta, b, ("obs", "next"), RELU_MARGIN, _draw_trained, KERNEL_SCALE)
        elif name in BRANCH:
            theta = _clear_biases(cfg, theta, b, ("obs",), FLIP_MARGIN, _draw_init)
        _INPUTS[name] = (cfg, B, theta, b, noise)
    return _INPUTS[name]


# ---- the fp64 statement, layer by layer ------------------------------------------------------------------------------------------
def layers_of(params, key, img_u8):
    """the oracle's SmallEncoder on u8 frames [N,H,W,3] -> ([pre-activation of layer 0..3], [ReLU output of layer 0..3],
    pooled [N,256]), in the dtype of `params`"""
    rec = []
    pooled = O.small_encoder_trunk(params, key, img_u8, layers=rec)
    return [p for p, _ in rec], [a for _, a in rec], pooled


class Margin:
    """observer "small" of O.observe_preactivations: the smallest |pre-activation| / the tensor's largest, over every conv layer of
    every encoder pass of the calls it watches"""

    def __init__(self):
        self.worst, self.seen = float("inf"), 0

    def see(self, pre):
        a = pre.detach().abs()
        self.worst = min(self.worst, float(a.min() / a.max()))
        self.seen += a.numel()


_REFERENCE = {}


def reference(name, dtype=torch.float64):
    """the oracle's side of a case, memoised and read-only: update_critics (update_high_utd for a case with "utd") from the case's
    parameters -> {"info", "aux", "st" (the TrainState after the call), "acts": {camera: [ReLU output of layer 0..3, numpy]} of the
    online encoder at the observations before the call, "margin": the Margin of the call, "obs_margin": the smallest
    |pre-activation| / the layer's largest of that encoder pass alone}"""
    key = (name, str(dtype))
    if key not in _REFERENCE:
        cfg, B, theta, b, noise = inputs(name)
        st = O.TrainState(cfg, {}, theta, dtype)
        tb, tn = AH.batch_to_torch(b, dtype), O.noise_to_torch(noise, dtype)
        acts, obs_margin = {}, float("inf")
        with torch.no_grad():
            for k in cfg.image_keys:
                pre, act, _ = layers_of(st.params, k, tb["obs"][k])
                acts[k] = [a.numpy() for a in act]
                obs_margin = min([obs_margin] + [float(p.abs().min() / p.abs().max()) for p in pre])
        m = Margin()
        with O.observe_preactivations({"small": m}):
            utd = CASES[name].get("utd")
            info, aux = O.update_critics(st, tb, tn) if utd is None else O.update_high_utd(st, tb, tn, utd)
        _REFERENCE[key] = {"info": info, "aux": aux, "st": st, "acts": acts, "margin": m, "obs_margin": obs_margin}
    return _REFERENCE[key]
