"""Shared by tests/test_optimizer_layouts_cpu.py (which proves what the layout table covers) and tests/test_optimizer_layouts_gpu.py
(which runs it): the arena layouts, schedules and inputs at which adam_ema_kernel (serl_amd/csrc/heads.hip) and frozen_ema_kernel
are compared element by element with the fp64 oracle's own optimizer -- O.apply_gradients, O.target_update, TrainState.lr_at,
driven with injected gradients, preset moments (TrainState.set_moments) and preset counts (TrainState.set_count).  Nothing
here restates Adam.

adam_ema_kernel gives four consecutive leaves to a thread and chooses per 4-vector between a 16-byte fast path and adam_elem; the
choice depends on where the vector lies relative to Pc (end of the critic optimizer's support), Pa0 and Pa1 (the actor
optimizer's support) and P - 1 (the temperature).  Which residues mod 4 those four take is a property of the layout, i.e. of
O.trainable_param_shapes: LAYOUTS is chosen so that every residue and every straddling vector occurs (the CPU test asserts it).

Inputs are conditioned so that the bounds, which are relative to the reference ELEMENT, are meaningful: an element's injected
gradients and its preset first moment share one sign (sign_pattern), so b1*mu + (1-b1)*g never cancels and the three float32
roundings of that expression stay three roundings of the result; a preset nu is exactly zero only where mu is and where the
element's gradients are exact zeros too (the state of an element that never saw a gradient), so that no second moment is a
float32 denormal other than an exact zero."""
import dataclasses

import numpy as np
import torch

from oracle import drq_oracle as O
import agent_helpers as AH

STATE = dict(image_keys=(), discount=0.99)
PIX = dict(H=32, W=32)
LOG_STDS_SEED = 17

# (id, oracle Config kwargs, those of them that leave the launcher's policy).  B = 4 everywhere; no update runs.
LAYOUTS = [
    ("state_w64_A1_S3_E3", dict(STATE, S=3, A=1, hidden=64, ensemble=3), {}),
    ("state_w64_A4_S4_E4", dict(STATE, S=4, A=4, hidden=64, ensemble=4), {}),
    ("state_w192_A5_S3_E3", dict(STATE, S=3, A=5, hidden=192, ensemble=3), {}),
    ("state_w320_A7_S2_E2", dict(STATE, S=2, A=7, hidden=320, ensemble=2), {}),
    ("state_w64_A7_S5_E5", dict(STATE, S=5, A=7, hidden=64, ensemble=5), {}),
    ("drq_1cam_S1_A3", dict(PIX, image_keys=("wrist",), S=1, A=3, hidden=64, ensemble=2), {}),
    ("drq_2cam_S3_A6", dict(PIX, image_keys=("front", "wrist"), S=3, A=6, hidden=64, ensemble=3), {}),
    ("drq_3cam_S5_A33", dict(PIX, image_keys=("a", "b", "c"), S=5, A=33, hidden=64, ensemble=2), {}),
    ("small_1cam_S3_A5", dict(PIX, image_keys=("wrist",), S=3, A=5, hidden=64, ensemble=3, encoder_type="small"), {}),
    ("uniform_state_w64_A5", dict(STATE, S=3, A=5, hidden=64, ensemble=2), {"std_parameterization": "uniform"}),
    ("adamw_state_w64_A4", dict(STATE, S=3, A=4, hidden=64, ensemble=2,
                                opt={"actor": {"weight_decay": 0.01}, "critic": {"weight_decay": 0.003},
                                     "temperature": {"weight_decay": 0.02}}), {}),
]
LAYOUT_IDS = [c[0] for c in LAYOUTS]
BOUNDARIES = ("Pc", "Pa0", "Pa1", "P-1")


def layout_config(case):
    """-> (oracle Config, the case's third entry)"""
    _, ckw, akw = case
    return O.Config(**ckw, **akw), dict(akw)


def layout_shapes(case):
    """{leaf (oracle name): shape} in arena order, from O.trainable_param_shapes alone (a "uniform" policy has actor/log_stds
    [A] where the others have the log-std Dense: actor_critic_nets.py:205-214)"""
    return dict(O.trainable_param_shapes(layout_config(case)[0]))


def slices_of(shapes):
    sl, off = {}, 0
    for k, shp in shapes.items():
        n = int(np.prod(shp)) if len(shp) else 1
        sl[k] = (off, off + n)
        off += n
    return sl, off


def boundaries(shapes):
    """Pc, Pa0, Pa1 as tests/test_agent_gpu.py derives them (test_adam_ema_injected, _check_grads), and P - 1"""
    sl, P = slices_of(shapes)
    last_actor = "actor/log_stds" if "actor/log_stds" in sl else "actor/logstd/bias"
    pc = sl.get("enc/proprio/ln/bias", sl["critic/head/bias"])[1]
    pa0 = sl.get("enc/proprio/dense/kernel", sl["actor/w1"])[0]
    return {"Pc": pc, "Pa0": pa0, "Pa1": sl[last_actor][1], "P-1": P - 1}


def boundary_vectors(shapes):
    """{boundary: the arena indices of the 4-vector that holds index `boundary` together with an index below it} -- the vectors
    adam_ema_kernel hands to adam_elem because they straddle; a boundary at a multiple of 4 has none"""
    _, P = slices_of(shapes)
    out = {}
    for name, x in boundaries(shapes).items():
        if x % 4:
            lo = x - x % 4
            out[name] = list(range(lo, min(lo + 4, P)))
    return out


def support(shapes):
    """{tx: [leaves inside that optimizer's support]}"""
    sl, P = slices_of(shapes)
    b = boundaries(shapes)
    return {"critic": [k for k, (lo, hi) in sl.items() if hi <= b["Pc"]],
            "actor": [k for k, (lo, hi) in sl.items() if lo >= b["Pa0"] and hi <= b["Pa1"]],
            "temperature": ["temp/lagrange"]}


# ---- parameters and moments ----------------------------------------------------------------------------------------------------
def layout_theta(case, seed):
    """-> (trunk, theta) float32, oracle names: O.init_params at `seed` (unit-sized LayerNorm scales, small kernels, perturbed
    biases), actor/log_stds for a uniform policy"""
    cfg, _ = layout_config(case)
    trunk, theta = O.init_params(cfg, seed)
    if "actor/log_stds" in theta:      # (the reference's zeros would leave std = 1 in every column)
        theta["actor/log_stds"] = np.random.default_rng(LOG_STDS_SEED + seed).uniform(-1.5, 0.5, cfg.A).astype(np.float32)
    return trunk, theta


def sign_pattern(P, seed=5):
    """+-1 per arena index: the sign an element's gradients and preset first moments carry"""
    return np.where(np.random.default_rng(seed).random(P) < 0.5, -1.0, 1.0).astype(np.float32)


def zero_pattern(P, seed=6):
    """-> (zero, tiny) boolean masks over the arena, disjoint: where every injected gradient is an exact zero / is 1e-20 (its
    square, 1e-40, leaves the float32 normal range): 3 % of the elements each; Pair adds one of each to every leaf of four
    elements or more."""
    r = np.random.default_rng(seed).random(P)
    return r < 0.03, (r >= 0.03) & (r < 0.06)


def gradient(rng, lo, hi, sign, zero, tiny, lo_exp=-9.0, hi_exp=3.0):
    """float32 gradient of arena range [lo, hi): |g| log-uniform in [1e-9, 1e3], the element's sign, exact zeros and 1e-20"""
    n = hi - lo
    g = (10.0 ** rng.uniform(lo_exp, hi_exp, n)).astype(np.float32)
    g[tiny[lo:hi]] = np.float32(1e-20)
    g[zero[lo:hi]] = 0.0
    return (g * sign[lo:hi]).astype(np.float32)


def preset_moments(rng, lo, hi, sign, zero):
    """-> (mu, nu) float32 of arena range [lo, hi): |mu| log-uniform in [1e-8, 1e-1] with the element's sign, nu log-uniform in
    [1e-12, 1e0]; both exactly zero on half of the elements whose gradients are exact zeros"""
    n = hi - lo
    mu = (10.0 ** rng.uniform(-8.0, -1.0, n)).astype(np.float32) * sign[lo:hi]
    nu = (10.0 ** rng.uniform(-12.0, 0.0, n)).astype(np.float32)
    never = zero[lo:hi] & (rng.random(n) < 0.5)
    mu[never] = 0.0
    nu[never] = 0.0
    return mu.astype(np.float32), nu


class Pair:
    """The oracle TrainState and the AgentCore of one layout, holding the same float32 parameters, targets and moments."""

    def __init__(self, case, B=4, presets=True, seed=42, cfg_override=None):
        self.case = case
        self.cfg = cfg = dataclasses.replace(layout_config(case)[0], **(cfg_override or {}))
        self.shapes = layout_shapes(case)
        self.sl, self.P = slices_of(self.shapes)
        self.b = boundaries(self.shapes)
        self.sup = support(self.shapes)
        self.names = {k: AH.product_name(k, cfg.image_keys) for k in self.shapes}
        trunk, theta = layout_theta(case, seed)
        _, target = layout_theta(case, seed + 1)
        self.st = O.TrainState(cfg, trunk, theta)
        self.st.target = O.to_torch(target, torch.float64)
        self.core = AH.make_core(cfg, B)
        AH.load_leaves(self.core, cfg, trunk, theta, target)
        self.sign = sign_pattern(self.P)
        self.zero, self.tiny = zero_pattern(self.P)
        for lo, hi in self.sl.values():
            if hi - lo >= 4:
                self.zero[lo + 1], self.tiny[lo + 1], self.zero[lo + 2], self.tiny[lo + 2] = True, False, False, True
        if presets:
            rng = np.random.default_rng(seed + 2)
            for tx in O.TX_NAMES:
                mus, nus = {}, {}
                for k in self.sup[tx]:
                    lo, hi = self.sl[k]
                    mus[k], nus[k] = preset_moments(rng, lo, hi, self.sign, self.zero)
                    if tx == "temperature":
                        mus[k] = np.abs(mus[k])     # the temperature's gradient is made positive: temperature_scalars
                    self.core.set(f"opt/{tx}/mu", self.names[k], mus[k])
                    self.core.set(f"opt/{tx}/nu", self.names[k], nus[k])
                self.st.set_moments(tx, mus, nus)

    def set_count(self, count):
        self.st.set_count(count)
        self.core.step = count

    # ---- one injected step on both sides ------------------------------------------------------------------------------------
    def _tree(self, g, tx, base):
        return {k: torch.tensor(g[self.sl[k][0] - base:self.sl[k][1] - base].astype(np.float64)).reshape(self.st.params[k].shape)
                for k in self.sup[tx]}

    def temperature_grad(self, excess):
        """-> (scalars for the S_LOGP_NEXT slot, the oracle's gradient): entropy H = target_entropy + excess (excess > 0: a
        positive gradient, lagrange.py / sac.py:223-234 with one row)"""
        H = self.cfg.target_entropy + excess
        sc = np.zeros(32, np.float32)
        sc[5] = np.float32(-H)
        lam = self.st.params["temp/lagrange"]
        return sc, torch.sigmoid(lam) * (-float(sc[5]) - self.cfg.target_entropy)

    def apply(self, which, g_critic=None, g_actor=None, excess=None):
        """which: SERL_NET_* bits (1 critic, 2 actor, 4 temperature).  The same float32 gradients go to the kernel (debug_set) and,
        as fp64, to O.apply_gradients; O.target_update follows a critic step (sac.py:284-285)."""
        grads = {}
        self.injected = {"critic": (g_critic, 0) if which & 1 else None, "actor": (g_actor, self.b["Pa0"]) if which & 2 else None}
        if which & 1:
            self.core.debug_set("g_critic", g_critic)
            grads["critic"] = self._tree(g_critic, "critic", 0)
        if which & 2:
            self.core.debug_set("g_actor", g_actor)
            grads["actor"] = self._tree(g_actor, "actor", self.b["Pa0"])
        if which & 4:
            sc, gt = self.temperature_grad(excess)
            self.core.debug_set("scalars", sc)
            grads["temperature"] = {"temp/lagrange": gt}
        O.apply_gradients(self.st, grads)
        if which & 1:
            O.target_update(self.st)
        self.core.apply(which)

    def read(self):
        """-> {section: {leaf: float32 array}} of the kernel's whole state (exact zeros outside an optimizer's support)"""
        out = {}
        for sec in ("params", "target_params") + tuple(f"opt/{tx}/{m}" for tx in O.TX_NAMES for m in ("mu", "nu")):
            out[sec] = {k: self.core.get(sec, self.names[k]) for k in self.shapes}
        return out

    def reference(self):
        """the oracle's state under the same keys as read(), fp64"""
        flat = lambda tree: {k: tree[k].numpy().reshape(-1).copy() for k in self.shapes}  # noqa: E731
        out = {"params": flat(self.st.params), "target_params": flat(self.st.target)}
        for tx in O.TX_NAMES:
            for m in ("mu", "nu"):
                out[f"opt/{tx}/{m}"] = flat(self.st.opt[tx][m])
        return out


# ---- the bounds (ISSUE: "Optimizer step and target EMA: exact checks on every arena layout") -------------------------------------
MU_REL = 2e-6          # three float32 roundings of b1*mu + (1-b1)*g, and 1 - 0.9f is 2.4e-7 away from 0.1
NU_REL = 3e-5          # float32's 1 - 0.999f is 1.3e-5 away from 0.001; the rest is rounding
STEP_REL = 1e-4        # 0.999f moves bc2 by <= 1.3e-5, one ulp of powf at t = 2 moves bc2 by 3e-5 and the step by half of it
DENORMAL = float(np.float32(1.401298464324817e-45))


def ulp(x):
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


def where_text(pair, leaf, idx):
    """names the arena index of element `idx` of `leaf`, and the boundary vector it lies in, for a failure message"""
    at = pair.sl[leaf][0] + int(idx)
    hits = [f"{b} = {x}" for b, x in pair.b.items() if x % 4 and x - x % 4 <= at < x - x % 4 + 4]
    return f"{leaf}[{int(idx)}] = arena {at}" + (f", in the vector straddling {' and '.join(hits)}" if hits else "")


class Worst:
    """worst error / bound per quantity, over everything a test run compared"""

    def __init__(self):
        self.v = {}

    def add(self, what, err, bound, raw=None):
        """err, bound: arrays; -> index of the worst element that does not hold `err <= bound`, or None when all hold.  A NaN error
        (a NaN from the kernel) does not hold: it counts as an infinite ratio."""
        err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0.0, 0.0, err / bound)
        ratio = np.where(np.isnan(ratio), np.inf, ratio)
        i = int(np.argmax(ratio)) if ratio.size else 0
        r = float(ratio[i]) if ratio.size else 0.0
        w = 0.0
        if raw is not None and np.size(raw):
            raw = np.asarray(raw, np.float64)
            w = float(np.max(np.where(np.isnan(raw), np.inf, raw)))
        cur = self.v.get(what, (0.0, 0.0))
        self.v[what] = (max(cur[0], r), max(cur[1], w))
        return None if r <= 1.0 else i

    def text(self):
        return "; ".join(f"{k}: worst err/bound {r:.3f}" + (f" (raw {w:.3g})" if w else "") for k, (r, w) in sorted(self.v.items()))


def check_step(pair, before, after, ref_before, ref_after, which, worst, tag):
    """Every element of every leaf after one apply: moments, the step itself, the target.  before / after: Pair.read() around the
    apply; ref_before / ref_after: Pair.reference() around it.  Raises AssertionError naming leaf, arena index and boundary
    vector."""
    tau = pair.cfg.tau
    bad = []

    def fail(what, k, i, got, ref, err, bound):
        bad.append(f"{tag} {what} {where_text(pair, k, i)}: got {got!r}, reference {ref!r}, err {err:.3e} > bound {bound:.3e}")

    for k in pair.shapes:
        for tx in O.TX_NAMES:
            inside = k in pair.sup[tx]
            for m, rel, floor in (("mu", MU_REL, DENORMAL), ("nu", NU_REL, 0.0)):
                sec = f"opt/{tx}/{m}"
                got, ref = after[sec][k].astype(np.float64), ref_after[sec][k]
                if not inside:      # outside the support: exact zeros
                    if np.any(after[sec][k].view(np.uint32) & 0x7FFFFFFF):
                        i = int(np.flatnonzero(after[sec][k])[0])
                        fail(sec + " outside the support", k, i, got[i], 0.0, abs(got[i]), 0.0)
                    continue
                err, bound = np.abs(got - ref), rel * np.abs(ref) + floor
                with np.errstate(divide="ignore", invalid="ignore"):
                    raw = np.where(ref != 0.0, err / np.abs(ref), 0.0)
                i = worst.add(sec.split("/")[-1], err, bound, raw)
                if i is not None:
                    fail(sec, k, i, got[i], ref[i], err[i], bound[i])
        # the step, from the two read-back parameters
        p0, p1 = before["params"][k], after["params"][k]
        d_got = p1.astype(np.float64) - p0.astype(np.float64)
        d_ref = ref_after["params"][k] - ref_before["params"][k]
        err = np.abs(d_got - d_ref)
        u = np.maximum(ulp(p0), ulp(p1))
        bound = STEP_REL * np.abs(d_ref) + 2.0 * u
        with np.errstate(divide="ignore", invalid="ignore"):      # reported: the relative error where the step spans >= 2^20 ulp of p
            raw = np.where(np.abs(d_ref) >= 1048576.0 * u, err / np.abs(d_ref), 0.0)
        i = worst.add("step", err, bound, raw)
        if i is not None:
            fail("step", k, i, d_got[i], d_ref[i], err[i], bound[i])
        # the target: an EMA of the read-back parameter after a critic step, untouched otherwise
        t0, t1 = before["target_params"][k], after["target_params"][k]
        if which & 1:
            a, c = p1.astype(np.float64) * tau, t0.astype(np.float64) * (1.0 - tau)
            want = a + c
            err = np.abs(t1.astype(np.float64) - want)
            # 2 ulp of the largest of the two products and their sum: each product rounds in its own binade (half an ulp each),
            # float32's 1 - tau is up to half an ulp of t away from 1 - 0.005, the sum rounds once.  Where the products cancel
            # the result is smaller than what was rounded, and its own ulp is no measure of a correct evaluation.
            unit = ulp(np.maximum(np.maximum(np.abs(a), np.abs(c)), np.abs(want)))
            bound = 2.0 * unit
            i = worst.add("target", err, bound, err / unit)
            if i is not None:
                fail("target", k, i, t1[i], want[i], err[i], bound[i])
        elif not np.array_equal(t0.view(np.uint32), t1.view(np.uint32)):
            i = int(np.flatnonzero(t0.view(np.uint32) != t1.view(np.uint32))[0])
            fail("target after an apply without the critic", k, i, t1[i], t0[i], abs(float(t1[i]) - float(t0[i])), 0.0)
    assert not bad, f"{len(bad)} elements out of bounds, first: " + " | ".join(bad[:6])


def check_moments_of_mixed_signs(pair, before, after, ref_after, worst, tag):
    """The critic's and the actor's moments after an apply whose gradients carry signs of their own, so that b1*mu and (1-b1)*g
    cancel on some elements.  mu: within 2e-6 of the LARGER of |mu before| and |g| (+ one denormal step) -- the float32 roundings of
    the two products are relative to the products, each no larger than these, whatever is left of their sum; where nothing cancels
    this is check_step's bound within a factor 10.  nu is a sum of non-negative terms: 3e-5 relative, as everywhere.  -> the smallest
    |mu after| / max(|mu before|, |g|) met (how far the cancellation went)."""
    bad, deepest = [], 1.0
    for tx in ("critic", "actor"):
        inj = pair.injected[tx]
        for k in pair.sup[tx]:
            lo, hi = pair.sl[k]
            g = np.zeros(hi - lo) if inj is None else np.abs(inj[0][lo - inj[1]:hi - inj[1]].astype(np.float64))
            size = np.maximum(np.abs(before[f"opt/{tx}/mu"][k].astype(np.float64)), g)
            for m, bound in (("mu", MU_REL * size + DENORMAL), ("nu", NU_REL * np.abs(ref_after[f"opt/{tx}/nu"][k]))):
                sec = f"opt/{tx}/{m}"
                got, ref = after[sec][k].astype(np.float64), ref_after[sec][k]
                err = np.abs(got - ref)
                i = worst.add(m + " (mixed signs)", err, bound)
                if i is not None:
                    bad.append(f"{tag} {sec} {where_text(pair, k, i)}: got {got[i]!r}, reference {ref[i]!r}, err {err[i]:.3e} > bound {bound[i]:.3e}")
            live = size > 0
            if live.any():
                deepest = min(deepest, float(np.min(np.abs(ref_after[f"opt/{tx}/mu"][k][live]) / size[live])))
    assert not bad, f"{len(bad)} elements out of bounds, first: " + " | ".join(bad[:6])
    return deepest


# ---- late counts and schedules --------------------------------------------------------------------------------------------------
COUNT_CASE = ("counts_state_w64", dict(STATE, S=3, A=5, hidden=64, ensemble=2), {})
COUNTS = [0, 1, 2, 9, 999, 1999, 2000, 2001, 99_999, 1_000_000, 2 ** 24 + 1]
COSINE = {"learning_rate": 1e-3, "warmup_steps": 100, "cosine_decay_steps": 1000}
COSINE_COUNTS = [99, 100, 101, 550, 999, 1000, 1001, 10 ** 6]
# (id, Config overrides, counts)
SCHEDULES = [
    ("default_warmup_2000", dict(warmup=2000, temp_warmup=0), COUNTS),         # SACAgent.create's defaults (sac.py:333-343)
    ("cosine_1000_warmup_100", dict(opt={tx: dict(COSINE) for tx in O.TX_NAMES}), COSINE_COUNTS),
    ("cosine_below_warmup", dict(opt={tx: {"warmup_steps": 50, "cosine_decay_steps": c} for tx, c in
                                      zip(O.TX_NAMES, (50, 20, 1))}), [0, 25, 49, 50, 51, 52, 10 ** 6]),
    ("three_schedules", dict(warmup=7, opt={"actor": dict(COSINE), "critic": {"learning_rate": 5e-4, "warmup_steps": 2000},
                                            "temperature": {"learning_rate": 1e-2, "warmup_steps": 0, "cosine_decay_steps": 3000}}),
     [0, 1, 99, 100, 550, 1000, 1999, 2000, 2999, 3000, 99_999]),
]
SCHEDULE_CASES = [(sid, c) for sid, _, counts in SCHEDULES for c in counts]
