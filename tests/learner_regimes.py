"""Shared by tests/test_learner_regimes_cpu.py, tests/test_learner_regimes_gpu.py and the two golden recipes
(tests/golden/make_golden_bc.py, tests/golden/make_golden_classifier_train.py): parameters, batches and shape tables of the
behaviour-cloning learner (csrc/bc.hip) and of the reward classifier's train step (csrc/classifier.hip) AWAY from
O.init_params / CO.make_params on uniform-noise frames, the only regime their other tests reach.  There the BC head's log_std
stays in [-1.5, 1.7] (std_min never binds, std_max in one entry), its tanh below 0.985, and every classifier logit in
[-0.51, -0.41].  tests/trained_regime.py is the same thing for the SAC / DrQ update chain.

The recipes are fixed by hand and their conditions are asserted on the fp64 oracles alone (tests/test_learner_regimes_cpu.py): if
a change of a recipe breaks one of them, the recipe is what changes."""
import math

import numpy as np
import torch

from oracle import classifier_oracle as CO
from oracle import drq_oracle as O
import bc_oracle as BO
import classifier_train_oracle as CT

# ================================================================================================================================
# behaviour cloning
# ================================================================================================================================
# column j % 4 of the log-std bias.  "both": below log(std_min) = -11.5 | inside | inside | above log(std_max) = 1.61.
# "max_only": no std_min column -- there the gradients of the std_min columns (proportional to 1 / std^2 = 1e10) are all that is left
# of every leaf below the heads, and w1, w2 and the proprio branch would not really be compared.
LOGSTD_CYCLES = {"both": (-14.0, -3.0, 0.3, 3.0), "max_only": (-3.0, 0.3, 3.0, -1.0)}
MEAN_CYCLE = (3.0, -0.4, 0.2, -2.5, 0.0)          # column j % 5: means well outside [-1, 1] and inside it
# hidden unit u % 8 of both tanh layers: bias +-13 -> |pre| > 9.02, tanh is exactly +-1 in fp32 (1 - t^2 = 0); bias +-7 -> 1 - t^2 of
# a few 1e-6 has a few fp32 steps of 6e-8 left (coarse); the other six eighths stay where they were
SAT_BIAS = (13.0, -13.0, 7.0, -7.0)
SAT_SHARE, COARSE_SHARE = 0.20, 0.20              # at least this share of the units of either layer, in every row
BC_SETS = ("both", "max_only")
BC_SEED, BC_BATCH_SEED, BC_MASK_SEED = 5, 9, 13
BC_CFG = O.Config(image_keys=("front", "wrist"), H=64, W=64, S=5, A=5)
BC_B = 8


def bc_trained_like(theta, cfg, which="both", seed=BC_SEED, sat_bias=SAT_BIAS):
    """theta (O.init_params' leaves) -> float32 BC theta of the trained regime.  Trunk, SLE and the camera heads stay as initialised."""
    rng = np.random.default_rng(seed)
    out = {k: np.array(v, np.float32) for k, v in BO.bc_theta(theta).items()}
    hd = cfg.hidden
    out["enc/proprio/ln/scale"] = rng.uniform(-0.5, 3.0, cfg.proprio_dim).astype(np.float32)      # mixed sign
    out["enc/proprio/ln/bias"] = rng.uniform(-1.0, 1.0, cfg.proprio_dim).astype(np.float32)
    out["actor/w1"] = (out["actor/w1"] * np.float32(1.5)).astype(np.float32)
    for b in ("actor/b1", "actor/b2"):
        v = (0.5 * rng.standard_normal(hd)).astype(np.float32)
        for r, s in enumerate(sat_bias):
            v[r::8] = s
        out[b] = v
    # the head kernels scale with 1 / sqrt(hidden): with a quarter of the hidden units at exactly +-1 a kernel of fixed scale would
    # shift whole columns by many units and the bias cycles would no longer decide which columns clip
    w = 1.0 / math.sqrt(hd)
    cyc = LOGSTD_CYCLES[which]
    out["actor/logstd/bias"] = np.array([cyc[j % 4] for j in range(cfg.A)], np.float32)
    out["actor/logstd/kernel"] = (0.2 * w * rng.standard_normal((hd, cfg.A))).astype(np.float32)
    out["actor/mean/bias"] = np.array([MEAN_CYCLE[j % 5] for j in range(cfg.A)], np.float32)
    out["actor/mean/kernel"] = (0.6 * w * rng.standard_normal((hd, cfg.A))).astype(np.float32)
    return out


def bc_clip_columns(cfg, which):
    """-> (columns clipped at std_min, unclipped, clipped at std_max) under LOGSTD_CYCLES[which]"""
    lo_b, hi_b = math.log(cfg.std_min), math.log(cfg.std_max)
    v = np.array([LOGSTD_CYCLES[which][j % 4] for j in range(cfg.A)])
    return np.where(v < lo_b)[0], np.where((v > lo_b) & (v < hi_b))[0], np.where(v > hi_b)[0]


def bc_theta(cfg, which, param_seed=42):
    """-> (trunk, regime theta)"""
    trunk, theta = O.init_params(cfg, param_seed)
    return trunk, bc_trained_like(theta, cfg, which)


def harden_bc_batch(state, action, mean, seed=BC_BATCH_SEED):
    """-> (state, action) float32.  States span tens, as raw robot proprioception does; of the action entries [b, j]: (b + j) % 4 == 0 is
    exactly +-1 (a demonstration at the action bound), == 1 lies within 1e-3 of `mean` (the policy's own mean there, float32), == 2 lies 3 to 5
    away from it, the rest stay uniform in [-1, 1].  Every column of two or more rows holds more than one kind (a column that held
    near-mean entries only would have a gradient that is all cancellation)."""
    rng = np.random.default_rng(seed)
    st = (np.asarray(state, np.float32) * np.float32(20.0)).astype(np.float32)
    a, m = np.array(action, np.float32), np.asarray(mean, np.float32).reshape(np.shape(action))
    kind = np.add.outer(np.arange(a.shape[0]), np.arange(a.shape[1])) % 4
    a[kind == 0] = np.where(a[kind == 0] >= 0, 1.0, -1.0)
    n = int((kind == 1).sum())
    a[kind == 1] = m[kind == 1] + rng.uniform(-1e-3, 1e-3, n).astype(np.float32)
    n = int((kind == 2).sum())
    a[kind == 2] = m[kind == 2] + (rng.uniform(3.0, 5.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    return st, a


def _keep_masks(cfg, B, seed):
    rng = np.random.default_rng(seed)
    return {k: (rng.random((B, cfg.sle_dim)) < 1.0 - cfg.dropout).astype(np.uint8) for k in cfg.image_keys}


def _noise_frames(cfg, B, seed):
    rng = np.random.default_rng(seed)
    return {k: rng.integers(0, 256, (B, cfg.H, cfg.W, 3), dtype=np.uint8) for k in cfg.image_keys}


_BC_INPUTS = {}


def bc_inputs(cfg, B, which, seed=BC_BATCH_SEED):
    """-> {"frames" {k: u8 [B, H, W, 3]}, "state", "action", "masks", "infer": {frames, state, action}}: the hardened batch of one
    update (near-mean actions relative to the train-mode mean under these masks) and of the inference calls (relative to the
    train=False mean); memoised, read-only"""
    key = (repr(cfg), B, which, seed)
    if key not in _BC_INPUTS:
        trunk, theta = bc_theta(cfg, which)
        st = BO.State(cfg, trunk, theta)
        out = {}
        for tag, s, masks in (("update", seed, _keep_masks(cfg, B, BC_MASK_SEED + seed)), ("infer", seed + 100, None)):
            rng = np.random.default_rng(s)
            frames = _noise_frames(cfg, B, s + 1)
            state = (20.0 * rng.standard_normal((B, cfg.S))).astype(np.float32)
            feats = BO.features(trunk, cfg, frames)
            with torch.no_grad():
                mean = BO.policy(st.params, cfg, feats, st.tensor(state), st.masks(masks))[0].numpy()
            _, action = harden_bc_batch(state / 20.0, rng.uniform(-1, 1, (B, cfg.A)), mean, s)
            out[tag] = {"frames": frames, "state": state, "action": action, "masks": masks}
        _BC_INPUTS[key] = dict(out["update"], infer=out["infer"])
    return _BC_INPUTS[key]


_BC_RUNS = {}


def bc_run(cfg, B, which, dtype=torch.float64):
    """one update from the regime theta on bc_inputs -> {"info", "grads" {leaf: numpy fp64}, "aux", "state" (after the step),
    "state0" (before)}; memoised, read-only"""
    key = (repr(cfg), B, which, str(dtype))
    if key not in _BC_RUNS:
        trunk, theta = bc_theta(cfg, which)
        st, st0 = BO.State(cfg, trunk, theta, dtype), BO.State(cfg, trunk, theta, dtype)
        inp = bc_inputs(cfg, B, which)
        feats = BO.features(trunk, cfg, inp["frames"], dtype)
        info, grads, aux = BO.update(st, feats, inp["state"], inp["action"], inp["masks"])
        _BC_RUNS[key] = {"info": info, "grads": {k: g.double().numpy() for k, g in grads.items()},
                         "aux": {k: v.double().numpy() for k, v in aux.items()}, "state": st, "state0": st0}
    return _BC_RUNS[key]


def column_errors(A, got, ref):
    """one head gradient leaf, per action column: max |got - ref| over the column / the column's own max |ref| -> [A] (nan where the
    reference column is exactly zero: those are compared for exact equality instead)"""
    got, ref = np.asarray(got, np.float64).reshape(-1, A), np.asarray(ref, np.float64).reshape(-1, A)
    scale = np.abs(ref).max(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(scale > 0, np.abs(got - ref).max(axis=0) / scale, np.nan)


def rel_err(got, ref):
    """leaf-normalised: max |got - ref| / max |ref|"""
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


# ---- the reference-derived golden (tests/golden/bc_regime_64.npz, tests/golden/make_golden_bc.py) -----------------------------------
BC_GOLDEN = "bc_regime_64"
# The golden is compared as tests/test_bc_gpu.py::_check_state compares, PARAMETERS after two Adam steps included, and Adam divides the
# scale of a gradient out.  A hidden unit whose tanh is exactly +-1 in float32 has a gradient of exactly 0 there and does not move, while
# in the reference's fp64 its 1 - t^2 of 1e-11 times an upstream 1e9 is far above Adam's eps and moves every weight of its row by lr; a
# unit with a coarse 1 - t^2 carries a float32 error of tens of percent into the second step's m / sqrt(v), which is tens of percent of lr.
# The float32 oracle itself misses the parameter rule on actor/w1 and actor/w2 with either kind of unit (measured: 99.9th percentile 6e-4
# against 1e-4), so no float32 implementation can meet it.  The golden's parameters therefore stop short of both: bias +-4.5 / +-3.5 puts
# half of the units at |t| > 0.99 with 1 - t^2 from 1e-5 to 1e-2, which float32 resolves to better than a percent.  The one-step tests
# against the oracle, which read gradients leaf by leaf, keep the +-13 / +-7.
BC_GOLDEN_SAT_BIAS = (4.5, -4.5, 3.5, -3.5)


# ... and a second golden, one update of the full regime (+-13 / +-7), compared on the infos and the Adam moments only: after one step
# the moments are the gradient, which float32 does reach.
BC_GOLDEN_SAT = "bc_regime_sat_64"
BC_GOLDEN_SAT_BIASES = {BC_GOLDEN: BC_GOLDEN_SAT_BIAS, BC_GOLDEN_SAT: SAT_BIAS}


def bc_golden_theta_transform(sat_bias):
    return lambda theta, cfg: bc_trained_like(theta, cfg, "both", sat_bias=sat_bias)


def bc_golden_batch_transform(cfg, param_seed, sat_bias):
    """the recipe's batch hook: a reference-format packed batch, hardened in place against the train=False mean of the regime theta
    (the keep-masks of the reference's run are drawn inside it and unknown beforehand)"""
    trunk, theta = O.init_params(cfg, param_seed)
    theta = bc_trained_like(theta, cfg, "both", sat_bias=sat_bias)
    st = BO.State(cfg, trunk, theta)

    def transform(pb, step):
        feats = BO.features(trunk, cfg, {k: v[:, 0] for k, v in pb["frames"].items()})
        with torch.no_grad():
            mean = BO.policy(st.params, cfg, feats, st.tensor(pb["state"][:, 0]))[0].numpy()
        s, a = harden_bc_batch(pb["state"], pb["action"], mean, BC_BATCH_SEED + step)
        pb["state"], pb["action"] = s, a
        return pb
    return transform


# ================================================================================================================================
# reward classifier
# ================================================================================================================================
CLS_KEYS, CLS_H, CLS_W, CLS_PARAM_SEED, CLS_FRAME_SEED, CLS_MASK_SEED = ("image",), 64, 64, 23, 704, 29
CLS_B = 16
# eval logits the head is fitted to, row by row; labels are the training loop's: ones, then zeros.  Bands: |l| < 1, 5 - 15, > 17 (fp32
# sigmoid is exactly 1 above 16.7: p - y = 0 on a correct positive), beyond +-90 (expf(|l|) overflows: p is exactly 0 on the negative side);
# each band holds correctly and wrongly labelled rows
CLS_TARGETS = (0.9, 0.9, 9.0, -7.0, 19.0, 18.0, 18.5, 20.0,          # label 1: correct, correct, correct, wrong, c, c, c, c
               -0.9, 0.9, -11.0, 8.0, -19.0, 18.0, -91.0, 92.0)      # label 0: c, w, c, w, c, w, c, w
CLS_ACCURACY = 11.0 / 16.0
# the train=True logits of the same rows under the injected keep-masks: the same bands and signs, other values.
# The case was softened twice against the float32 oracle's 2e-5 yardstick (the oracle in float32 throughout, frozen trunk included; the
# figures are its worst gradient leaf).  A first table had as many wrong positives as wrong negatives and logits up to 130: the gradient of
# head/dense1/bias, mean(p - y), cancelled to 0.009 and missed by 1.5e-4; the wrong rows are now mostly negatives.  A second had logits of
# 0.3 - 0.8, 19 - 45 and +-93 - 100 and measured 2.7e-5: the float32 trunk's error of 1e-6 reaches the |logit| < 1 rows, where p (1 - p) is
# 0.25, through the kernel that also makes the largest logit, so every band now sits at the near end of its range (0.9, 18 - 20, 91 - 92).
# What is left depends on the frames: of the frame seeds 702 - 705 the float32 oracle measures 7.8e-6, 8.9e-6, 5.4e-6 and 2.1e-5, and 704 is
# used (6.5e-6 with one thread).
CLS_TRAIN_TARGETS = (0.9, 0.9, 6.0, -12.0, 18.0, 20.0, 19.0, 18.5, -0.9, 0.9, -8.0, 13.0, -18.0, 19.0, -92.0, 91.0)
# the six rows of the golden's batch (the B of classifier_train_one_cam_64), both epochs
CLS_GOLDEN, CLS_GOLDEN_B = "regime_one_cam_64", 6
CLS_GOLDEN_TARGETS = (95.0, -8.0, 0.5, -120.0, 20.0, -0.3)           # labels 1 1 1 0 0 0: c, w, c | c, w, c -> accuracy 4 / 6
GRID = 2.0 ** -10   # the fitted kernel is rounded to this grid: last-bit differences of a LAPACK build cannot change the parameters


def structured_frames(keys, H, W, B, seed):
    """{k: u8 [B, 1, H, W, 3]}: per row one colour and one sinusoid pattern, so that the frozen trunk separates the rows (on uniform
    noise every row gives nearly the same features)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = {}
    for k in keys:
        col = rng.uniform(40.0, 215.0, (B, 1, 1, 3))
        fx, fy = rng.integers(0, 7, (B, 1, 1, 1)), rng.integers(0, 7, (B, 1, 1, 1))
        ph, amp = rng.uniform(0.0, 2 * np.pi, (B, 1, 1, 3)), rng.uniform(20.0, 110.0, (B, 1, 1, 3))
        v = col + amp * np.sin(2 * np.pi * (fx * x[None, :, :, None] / W + fy * y[None, :, :, None] / H) + ph)
        out[k] = np.clip(np.rint(v), 0, 255).astype(np.uint8)[:, None]
    return out


def cls_base_params(keys=CLS_KEYS, H=CLS_H, W=CLS_W, seed=CLS_PARAM_SEED):
    """CO.make_params with the head's LayerNorm scale of mixed sign (ReLU kills whole columns of every row's gradient)"""
    p = CO.make_params(keys, H, W, seed)
    rng = np.random.default_rng(seed + 2000)
    p["head/ln/scale"] = rng.uniform(-0.5, 2.0, 256).astype(np.float32)
    p["head/ln/bias"] = rng.uniform(-0.3, 0.3, 256).astype(np.float32)
    return p


def _th(params):
    return {k: torch.tensor(np.asarray(v), dtype=torch.float64) for k, v in params.items() if not k.startswith("trunk/")}


def fit_head(params, keys, frames_list, targets_list, masks_list=None, train_targets_list=None):
    """-> params whose train=False logits on the given batches ({k: u8 [B, H, W, 3]}) are `targets` (and, with masks, whose train=True
    logits under those keep-masks are `train_targets`).  Two steps, both rounded to GRID so that the float32 parameters do not depend on
    the last bits of a LAPACK build: every camera's bottleneck bias cancels the mean of its Dense output over the rows (what the rows
    share would otherwise be nearly all of it, and the LayerNorm behind it would hand every row the same code); head/dense1/kernel is
    the minimum-norm kernel through the targets, head/dense1/bias is 0.25."""
    out = dict(params)
    feats = [CT.features(params, keys, fr) for fr in frames_list]
    th = _th(out)
    for k in keys:
        z = torch.cat([O.sle(f[k], th[f"enc/{k}/sle"]) @ th[f"enc/{k}/dense/kernel"] for f in feats])
        out[f"enc/{k}/dense/bias"] = (np.rint(-z.mean(0).numpy() / GRID) * GRID).astype(np.float32)
    th = _th(out)
    h = [CT.hidden(th, keys, f).numpy() for f in feats]
    t = [np.asarray(v, np.float64) for v in targets_list]
    if masks_list is not None:
        for f, m, tt in zip(feats, masks_list, train_targets_list):   # (None: that row's train logit is left free)
            rows = [i for i, v in enumerate(tt) if v is not None]
            h.append(CT.hidden(th, keys, f, m).numpy()[rows])
            t.append(np.array([tt[i] for i in rows], np.float64))
    bias = 0.25
    w, *_ = np.linalg.lstsq(np.concatenate(h), np.concatenate(t) - bias, rcond=None)
    out["head/dense1/kernel"] = (np.rint(w / GRID) * GRID).astype(np.float32).reshape(256, 1)
    out["head/dense1/bias"] = np.array([bias], np.float32)
    return out


def cls_labels(B):
    return np.concatenate([np.ones(B // 2), np.zeros(B - B // 2)]).astype(np.float32)


_CLS = {}


def cls_regime():
    """-> {"params", "frames" {k: u8 [B, 1, H, W, 3]}, "labels" [B], "masks"}; memoised, read-only"""
    if "regime" not in _CLS:
        frames = structured_frames(CLS_KEYS, CLS_H, CLS_W, CLS_B, CLS_FRAME_SEED)
        rng = np.random.default_rng(CLS_MASK_SEED)
        masks = {k: rng.random((CLS_B, 4096)) < 0.9 for k in CLS_KEYS}
        masks["head"] = rng.random((CLS_B, 256)) < 0.9
        params = fit_head(cls_base_params(), CLS_KEYS, [{k: v[:, 0] for k, v in frames.items()}], [CLS_TARGETS], [masks], [CLS_TRAIN_TARGETS])
        _CLS["regime"] = {"params": params, "frames": frames, "labels": cls_labels(CLS_B), "masks": masks}
    return _CLS["regime"]


def cls_run(dtype=torch.float64):
    """one train step in the regime -> {"loss", "accuracy", "eval" [B], "train" [B] logits, "grads"}; memoised, read-only"""
    key = ("run", str(dtype))
    if key not in _CLS:
        r = cls_regime()
        _CLS[key] = cls_step(r["params"], CLS_KEYS, r["frames"], r["labels"], r["masks"], dtype)
    return _CLS[key]


def cls_step(params, keys, frames, labels, masks, dtype=torch.float64):
    """one train step of the oracle in `dtype`, the frozen trunk included"""
    st = CT.State(params, keys, dtype=dtype)
    feats = CT.features(params, keys, {k: v[:, 0] for k, v in frames.items()}, dtype)
    th = {k: torch.tensor(np.asarray(v), dtype=dtype) for k, v in params.items() if not k.startswith("trunk/")}
    with torch.no_grad():
        train = CT.forward(th, keys, feats, masks).double().numpy().reshape(-1)
    loss, acc, ev, grads = CT.train_step(st, feats, labels, masks)
    return {"loss": loss, "accuracy": acc, "eval": ev.reshape(-1), "train": train, "grads": grads, "state": st}


def cls_golden_frames(keys, H, W, B, epochs, seed=750):
    """the golden's frame builder: epoch e -> structured frames of its own"""
    return [structured_frames(keys, H, W, B, seed + e) for e in range(epochs)]


def cls_golden_params(keys, H, W, pseed, cropped):
    """the golden's theta transform: cls_base_params with the head fitted through the cropped frames of every epoch"""
    return fit_head(cls_base_params(keys, H, W, pseed), keys, cropped, [CLS_GOLDEN_TARGETS] * len(cropped))


# ================================================================================================================================
# edge tables: the smallest images the library takes, one camera unless the row is about cameras
# ================================================================================================================================
MAX_CAMS = 4    # SERL_MAX_CAMS (include/serl_mi355.h)
BC_TRIP = 256   # rows of one trip of bc_gauss_head_kernel's loop (one workgroup, rows strided over its 256 threads)
CLS_ROWS_PER_WG, CLS_INFO_TRIP = 4, 256
# (id, cameras, B, A, S)
BC_EDGES = [
    ("B1", 1, 1, 4, 5), ("B7", 1, 7, 4, 5), ("B255", 1, 255, 4, 5), ("B257", 1, 257, 4, 5), ("B520", 1, 520, 4, 5),
    ("A1", 1, 7, 1, 5), ("A33", 1, 7, 33, 5), ("A64", 1, 9, 64, 5),
    ("S1", 1, 7, 4, 1), ("S65", 1, 7, 4, 65), ("S130", 1, 7, 4, 130),
    ("cams3", 3, 7, 4, 5), ("cams4", MAX_CAMS, 7, 4, 5),
]
BC_A_REFUSED = 65
# (id, cameras, B)
CLS_EDGES = [("B1", 1, 1), ("B2", 1, 2), ("B5", 1, 5), ("B7", 1, 7), ("B257", 1, 257), ("B300", 1, 300), ("cams3", 3, 5), ("cams4", MAX_CAMS, 7)]
EDGE_HW = 32


def bc_edge_cfg(row):
    _, n_cam, B, A, S = row
    return O.Config(image_keys=tuple("abcd"[:n_cam]), H=EDGE_HW, W=EDGE_HW, S=S, A=A), B


_EDGE = {}


def cls_edge(row):
    """-> (keys, params, frames, labels, masks) of one CLS_EDGES row: structured frames, the mixed-sign head, the last kernel 40
    times CO.make_params' so the logits leave (-1, 1); labels alternate (B = 1: all one class)"""
    name, n_cam, B = row
    if name not in _EDGE:
        keys = tuple("abcd"[:n_cam])
        p = cls_base_params(keys, EDGE_HW, EDGE_HW, 31)
        p["head/dense1/kernel"] = (p["head/dense1/kernel"] * np.float32(40.0)).astype(np.float32)
        rng = np.random.default_rng(41 + B)
        masks = {k: rng.random((B, 4096)) < 0.9 for k in keys}
        masks["head"] = rng.random((B, 256)) < 0.9
        labels = (np.arange(B) % 2 == 0).astype(np.float32)
        _EDGE[name] = (keys, p, structured_frames(keys, EDGE_HW, EDGE_HW, B, 43 + B), labels, masks)
    return _EDGE[name]


# ---- the HIP learners of a table row (GPU tests) -----------------------------------------------------------------------------------
def bc_agent(cfg, B, trunk, theta):
    from serl_amd import jaxrng as J
    from serl_amd.agents.bc import BCAgent
    agent = BCAgent(cfg.image_keys, cfg.H, cfg.W, cfg.S, cfg.A, seed_key=J.prngkey(0), max_batch=B)
    agent.load_flat(trunk)
    agent.load_flat(theta)
    return agent


def bc_batch(frames, state, action):
    t = lambda a: torch.tensor(np.ascontiguousarray(a), device="cuda")  # noqa: E731
    return {"observations": dict({k: t(v) for k, v in frames.items()}, state=t(state)), "actions": t(action)}


def classifier(keys, H, W, params, max_batch, lr=1e-4):
    from serl_amd.networks.reward_classifier import Classifier
    return Classifier(keys, H, W, max_batch=max_batch, trainable=True, learning_rate=lr).load_flat(params)
