"""Shared by tests/test_trained_regime_cpu.py, tests/test_trained_regime_gpu.py and tests/golden/make_golden_update_trained.py:
parameters and batches of the regime a trained SERL policy lives in, which O.init_params + AH.synth_batch do not reach (there
log_std stays in [-3, 1.9]: std_max binds in a few percent of the entries, std_min never; |u| < 3; |Q| < 1; alpha = 0.01) --
exp(log_std) clipped on both sides of [std_min, std_max] in whole columns, tanh saturated to exactly +-1 in fp32 (and, in one case,
exp(2|u|) beyond the fp32 range), |Q| of tens, alpha from 2e-3 to 4, terminal / non-terminal / mixed masks, rewards of both signs
and stored actions at exactly +-1, with a target copy that differs from the online parameters.

The recipe is fixed by hand and its conditions are asserted on the fp64 oracle alone (tests/test_trained_regime_cpu.py): if a
change of the recipe breaks one of them, the recipe is what changes."""
import numpy as np
import torch

from oracle import drq_oracle as O
import agent_helpers as AH
import golden_replay as GR

UPDATE_GOLDEN = ("sac_state_A4", "drq_64_A5")

LOGSTD_CYCLE = (-14.0, -3.0, 0.5, 3.0)     # column j % 4: below log(std_min) = -11.5 | inside | inside | above log(std_max) = 1.61
# column j % 5: tanh(12) is exactly 1 in fp32 (|u| > 9), tanh(-7) = -(1 - 1.7e-6) leaves a coarse fp32 1 - a^2, the rest stay below 2
MEAN_CYCLE = (12.0, -7.0, 0.2, 0.0, -1.5)
MEAN_CYCLE_OVERFLOW = (12.0, -60.0, 0.2, 60.0, -1.5)   # exp(2 * 60) is beyond the fp32 range: only the stable softplus survives
TRANSFORM_SEED, TARGET_SEED, BATCH_SEED = 5, 11, 9


def _is_ln(name, what):
    parts = name.split("/")
    return parts[-1] == what and parts[-2] in ("ln", "ln1", "ln2")


def trained_like(theta, cfg, seed=TRANSFORM_SEED, lam=0.5, mean_cycle=MEAN_CYCLE):
    """theta (O.init_params' leaves) -> float32 theta of the trained regime.  SLE, conv and dense kernels stay as initialised."""
    rng = np.random.default_rng(seed)
    out = {k: np.array(v, np.float32) for k, v in theta.items()}
    for k, v in out.items():
        if _is_ln(k, "scale"):
            out[k] = rng.uniform(-0.5, 3.0, v.shape).astype(np.float32)
        elif _is_ln(k, "bias"):
            out[k] = rng.uniform(-1.0, 1.0, v.shape).astype(np.float32)
        elif k in ("actor/b1", "actor/b2", "critic/b1", "critic/b2") or (k.startswith("enc/") and k.endswith("/dense/bias")):
            out[k] = rng.standard_normal(v.shape).astype(np.float32)
    # the head kernels scale with 1 / sqrt(hidden): the hidden activations are of order 1 and, with biases of order 1 in front of the
    # LayerNorms, nearly the same in every row, so a kernel of fixed scale would shift a whole column by many units at random and
    # the bias cycles below would no longer decide which columns clip and saturate
    A, w = cfg.A, 1.0 / np.sqrt(cfg.hidden)
    out["actor/logstd/bias"] = np.array([LOGSTD_CYCLE[j % 4] for j in range(A)], np.float32)
    out["actor/logstd/kernel"] = (0.3 * w * rng.standard_normal(out["actor/logstd/kernel"].shape)).astype(np.float32)
    out["actor/mean/kernel"] = (0.6 * w * rng.standard_normal(out["actor/mean/kernel"].shape)).astype(np.float32)
    out["actor/mean/bias"] = np.array([mean_cycle[j % 5] for j in range(A)], np.float32)
    out["critic/head/kernel"] = (out["critic/head/kernel"] * np.float32(40.0)).astype(np.float32)
    out["critic/head/bias"] = np.full(out["critic/head/bias"].shape, 35.0, np.float32)
    out["temp/lagrange"] = np.float32(lam)
    return out


def perturb_target(theta, cfg=None, seed=TARGET_SEED):
    """the target copy of a trained_like theta: another head bias and a weaker second layer, so that a kernel reading the online
    critic where the target belongs shows.  The generator of the goldens and the tests use this one function."""
    rng = np.random.default_rng(seed)
    out = {k: np.array(v, np.float32) for k, v in theta.items()}
    hb = out["critic/head/bias"]
    out["critic/head/bias"] = (hb + 0.05 * rng.standard_normal(hb.shape)).astype(np.float32)
    out["critic/w2"] = (out["critic/w2"] * np.float32(0.9)).astype(np.float32)
    return out


def clip_columns(cfg):
    """-> (columns clipped low, unclipped, clipped high) of the policy head under LOGSTD_CYCLE"""
    j = np.arange(cfg.A) % 4
    return np.where(j == 0)[0], np.where((j == 1) | (j == 2))[0], np.where(j == 3)[0]


def harden_batch(b, mode, seed=BATCH_SEED):
    """on an AH.synth_batch (or a reference-format sample: the same three fields), in place; -> b"""
    B = b["reward"].shape[0]
    m = np.zeros(B, np.float32)
    if mode == "one":
        m[:] = 1.0
    elif mode == "mixed":
        m[::3] = 1.0
    else:
        assert mode == "zero", mode
    b["mask"] = m
    b["reward"] = (20.0 * np.random.default_rng(seed).standard_normal(B)).astype(np.float32)
    a = np.array(b["action"], np.float32)
    a[::4] = np.sign(a[::4])
    b["action"] = a
    return b


def theta_pair(cfg, lam, mean_cycle=MEAN_CYCLE, param_seed=42):
    """-> (trunk, online theta, target theta)"""
    trunk, theta = O.init_params(cfg, param_seed)
    theta = trained_like(theta, cfg, lam=lam, mean_cycle=mean_cycle)
    return trunk, theta, perturb_target(theta, cfg)


def oracle_state(cfg, lam, dtype=torch.float64, mean_cycle=MEAN_CYCLE, param_seed=42):
    trunk, theta, target = theta_pair(cfg, lam, mean_cycle, param_seed)
    st = O.TrainState(cfg, trunk, theta, dtype)
    st.target = O.to_torch(target, dtype)
    return st


def pair(cfg, B, lam, fuse=None, mean_cycle=MEAN_CYCLE):
    """AH.make_pair in the trained regime -> (oracle TrainState, AgentCore): trained_like parameters in both, perturb_target in
    both target copies.  fuse: None = the default chain, True / False = SERL_CHAIN_FUSE 1 / 0."""
    trunk, theta, target = theta_pair(cfg, lam, mean_cycle)
    core = AH.load_leaves(AH.make_core(cfg, B, fuse=fuse), cfg, trunk, theta, target)
    return oracle_state(cfg, lam, torch.float64, mean_cycle), core


def _state(A, hidden=256, **kw):
    return O.Config(image_keys=(), S=10, A=A, ensemble=10, discount=0.99, hidden=hidden, warmup=4, temp_warmup=0, **kw)


MODES3 = ((-6.0, "zero"), (4.0, "one"), (0.5, "mixed"))
# (id, oracle Config, batch rows, ((temp/lagrange, mask mode), ...), mean-bias cycle).  Every case has A >= 4: with A = 3 the
# log_std cycle never reaches the high clip.  lagrange -6 / 0.5 / 4 = alpha 2.5e-3 / 0.97 / 4.02.
CASES = [
    ("state_A4", _state(4), 48, MODES3, MEAN_CYCLE),
    ("state_A7_backup_all", _state(7, backup_entropy=True, subsample=None), 40, MODES3, MEAN_CYCLE),
    ("state_A5_overflow", _state(5), 7, ((0.5, "mixed"),), MEAN_CYCLE_OVERFLOW),
    ("frozen_A5", O.Config(image_keys=("wrist",), H=64, W=64, S=5, A=5), 8, ((-6.0, "zero"), (4.0, "one")), MEAN_CYCLE),
    ("small_A4_w320", O.Config(image_keys=("wrist",), H=33, W=47, S=5, A=4, hidden=320, ensemble=3, encoder_type="small"), 7,
     ((0.5, "mixed"),), MEAN_CYCLE),
    ("state_A4_w64", _state(4, hidden=64), 65, ((4.0, "one"),), MEAN_CYCLE),      # the 64-wide LayerNorm kernel
    ("state_A4_w192", _state(4, hidden=192), 65, ((4.0, "one"),), MEAN_CYCLE),    # the strided generic row
]
RUNS = [(c, lam, mode) for c in CASES for lam, mode in c[3]]
RUN_IDS = [f"{c[0]}-lam{lam:g}-{mode}" for c, lam, mode in RUNS]


def second_utd(B):
    """the UTD > 1 of a case: 2, or the smallest divisor of an odd row count (sac.py:561-563 refuses a batch utd does not divide)"""
    return next(u for u in range(2, B + 1) if B % u == 0)


def inputs(case, mode, utd=1):
    """-> (batch of the critic call, its noise, batch of the high-UTD call, its noise), numpy"""
    _, cfg, B, _, _ = case
    return (harden_batch(AH.synth_batch(cfg, B, seed=3), mode), O.make_noise(cfg, B, seed=7),
            harden_batch(AH.synth_batch(cfg, B, seed=4), mode, seed=BATCH_SEED + 1), O.make_noise(cfg, B, seed=8, utd_ratio=utd))


# ---- the reference-derived goldens (tests/golden/trained_update_*.npz, tests/golden/make_golden_update_trained.py) ------------
def golden_batch_transform(mode):
    def transform(pb, step):
        return harden_batch(pb, mode, seed=BATCH_SEED + step)
    return transform


def update_golden(name):
    """tests/golden/trained_update_<name>.npz, its batches hardened as the generator hardened them -> (golden, online theta,
    target theta, trunk)"""
    g, meta, _ = GR.load_variant("trained_update", name)
    tr = meta["trained"]
    assert tr["transform"] == "trained_like" and tr["seed"] == TRANSFORM_SEED and tr["target_seed"] == TARGET_SEED
    bt = golden_batch_transform(tr["mask_mode"])
    for i, step in enumerate(g["steps"]):
        bt(step["batch"], i)
    trunk, theta, target = theta_pair(g["cfg"], tr["lam"], param_seed=g["meta"]["param_seed"])
    return g, theta, target, trunk


# ---- the oracle's side of a run, computed once per (case, mode, dtype) and shared by the tests --------------------------------
class Snapshot:
    """the part of an oracle TrainState tests/test_agent_gpu.py::_compare_state reads, frozen at one point of a run"""

    def __init__(self, st):
        self.params = {k: v.clone() for k, v in st.params.items()}
        self.target = {k: v.clone() for k, v in st.target.items()}
        self.step = st.step


def policy_pre(st, b, noise, side, mask_name):
    """-> (mean, log_std) [B, A] of the online policy at the batch's observations (side "obs") or next observations ("next")"""
    cfg = st.cfg
    with torch.no_grad():
        feats = O.features(st, b[side])
        enc = O.encode(st.params, cfg, feats, b["state" if side == "obs" else "next_state"], drop_masks=noise[mask_name],
                       stop_gradient=True)
        th = st.params
        h = O.policy_mlp(th, cfg, enc)
        return h @ th["actor/mean/kernel"] + th["actor/mean/bias"], h @ th["actor/logstd/kernel"] + th["actor/logstd/bias"]


_RUNS = {}


def reference_run(case, lam, mode, dtype=torch.float64):
    """update_critics, then update_high_utd(1), from oracle_state -> {"info1", "aux1", "after1", "info2", "aux2", "after2",
    "pre": {eps name: (mean, log_std, eps)} of the three policy evaluations}; memoised, read-only"""
    key = (case[0], lam, mode, str(dtype))
    if key not in _RUNS:
        _, cfg, B, _, cyc = case
        st = oracle_state(cfg, lam, dtype, cyc)
        b1, n1, b2, n2 = inputs(case, mode)
        tb1, tn1, tb2, tn2 = AH.batch_to_torch(b1, dtype), O.noise_to_torch(n1, dtype), AH.batch_to_torch(b2, dtype), O.noise_to_torch(n2, dtype)
        pre = {"eps_next": policy_pre(st, tb1, tn1, "next", "mask_next") + (tn1["eps_next"],)}
        r = {"pre": pre}
        r["info1"], r["aux1"] = O.update_critics(st, tb1, tn1)
        r["after1"] = Snapshot(st)
        pre["eps_pi"] = policy_pre(st, tb2, tn2, "obs", "mask_obs_pi") + (tn2["eps_pi"],)
        pre["eps_temp"] = policy_pre(st, tb2, tn2, "next", "mask_next_temp") + (tn2["eps_temp"],)
        r["info2"], r["aux2"] = O.update_high_utd(st, tb2, tn2, 1)
        r["after2"] = Snapshot(st)
        _RUNS[key] = r
    return _RUNS[key]


def reference_run_utd(case, lam, mode, utd):
    """update_high_utd(utd) from oracle_state, fp64 -> {"info", "aux", "after"}; memoised, read-only"""
    key = (case[0], lam, mode, "utd", utd)
    if key not in _RUNS:
        _, cfg, B, _, cyc = case
        st = oracle_state(cfg, lam, torch.float64, cyc)
        _, _, b2, n2 = inputs(case, mode, utd)
        info, aux = O.update_high_utd(st, AH.batch_to_torch(b2, torch.float64), O.noise_to_torch(n2, torch.float64), utd)
        _RUNS[key] = {"info": info, "aux": aux, "after": Snapshot(st)}
    return _RUNS[key]


POLICY_HEAD_LEAVES = ("actor/mean/kernel", "actor/mean/bias", "actor/logstd/kernel", "actor/logstd/bias")


def column_errors(cfg, got, ref):
    """one policy-head gradient leaf, per action column: max |got - ref| over the column / the column's own max |ref| -> [A]
    (nan where the reference column is exactly zero: those are compared for exact equality instead)"""
    got, ref = np.asarray(got, np.float64).reshape(-1, cfg.A), np.asarray(ref, np.float64).reshape(-1, cfg.A)
    scale = np.abs(ref).max(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(scale > 0, np.abs(got - ref).max(axis=0) / scale, np.nan)
