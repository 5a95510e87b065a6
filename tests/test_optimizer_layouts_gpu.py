"""GPU: adam_ema_kernel and frozen_ema_kernel (serl_amd/csrc/heads.hip) element by element against the fp64 oracle's own optimizer
(O.apply_gradients / O.target_update / TrainState.lr_at), with injected gradients, preset moments and preset counts
(tests/optimizer_cases.py; what its layout table covers is proved in tests/test_optimizer_layouts_cpu.py).

1. Layout table: every element of every leaf of eleven arena layouts after critic, actor + temperature, critic applies --
   mu within 2e-6 relative (+ one float32 denormal step), nu within 3e-5 relative, the step p_after - p_before within
   1e-4 |step| + 2 ulp(p), the target within 2 ulp of the EMA of the read-back parameter (the ulp of the largest of p tau, t (1 - tau)
   and their sum: optimizer_cases.check_step says why; bit-identical after an apply without the critic), exact zeros outside an optimizer's support.  A failure names the leaf, the arena index and the boundary vector.
2. Late counts and schedules: one injected step at counts up to 2^24 + 1 on four schedules; the reported rates within one float32
   ulp of lr_at, exactly 0.0 at and past the end of a cosine decay and that optimizer's leaves bit-identical; clip_grad_norm at
   0.5x, 2x, 1e6x the clip and on an all-zero gradient.
3. The deferred target-trunk EMA (frozen_ema_kernel): N pending steps at once against N flushes of one step (bit for bit) and
   against the fp64 closed form; a set of an online trunk leaf between applies; a snapshot and a checkpoint taken with steps
   pending; update_high_utd(utd = 3) counts three.
4. The BC and classifier slices (AdamSlice::apply, heads.h): the step from the read-back moments at counts 0, 999 and 10^6.

The measured worst values and the mutations that these tests catch: DESIGN.md section 2."""
import numpy as np
import pytest

from oracle import drq_oracle as O
import agent_helpers as AH
import optimizer_cases as OC

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. the layout table ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", OC.LAYOUTS, ids=OC.LAYOUT_IDS)
def test_every_element_of_every_layout(gpu, case):
    pair = OC.Pair(case)
    b = pair.b
    rng = np.random.default_rng(11)
    worst = OC.Worst()
    before, ref_before = pair.read(), pair.reference()
    for sec in before:          # what was preloaded is what is there: float32 values on both sides
        for k in pair.shapes:
            assert np.array_equal(before[sec][k].astype(np.float64), ref_before[sec][k]), (sec, k)
    assert any(not np.array_equal(before["params"][k], before["target_params"][k]) for k in pair.shapes)
    for it, which in enumerate((1, 6, 1)):
        if which == 1:
            pair.apply(1, g_critic=OC.gradient(rng, 0, b["Pc"], pair.sign, pair.zero, pair.tiny))
        else:
            pair.apply(6, g_actor=OC.gradient(rng, b["Pa0"], b["Pa1"], pair.sign, pair.zero, pair.tiny), excess=0.75)
        after, ref_after = pair.read(), pair.reference()
        OC.check_step(pair, before, after, ref_before, ref_after, which, worst, f"{case[0]} apply {it} (which = {which})")
        before, ref_before = after, ref_after
    assert pair.core.step == pair.st.step == 3
    print(f"{case[0]}: P = {pair.P}, boundaries {b}, straddling vectors {sorted(OC.boundary_vectors(pair.shapes))}; {worst.text()}")


@pytest.mark.parametrize("case", [c for c in OC.LAYOUTS if c[0] in ("state_w64_A7_S5_E5", "drq_1cam_S1_A3")], ids=lambda c: c[0])
def test_first_moments_where_momentum_and_gradient_cancel(gpu, case):
    """test_every_element_of_every_layout gives an element's gradients the sign of its preset mu, because its mu bound is relative
    to the element.  Here every apply draws fresh signs, so b1*mu + (1-b1)*g cancels on some elements (asserted: to below 1 % of the
    larger term), and the moments are held to the bound of optimizer_cases.check_moments_of_mixed_signs."""
    pair = OC.Pair(case)
    b = pair.b
    rng = np.random.default_rng(14)
    worst, deepest = OC.Worst(), 1.0
    before = pair.read()
    for it, which in enumerate((1, 6, 1)):
        sign = np.where(rng.random(pair.P) < 0.5, -1.0, 1.0).astype(np.float32)
        if which == 1:
            pair.apply(1, g_critic=OC.gradient(rng, 0, b["Pc"], sign, pair.zero, pair.tiny))
        else:
            pair.apply(6, g_actor=OC.gradient(rng, b["Pa0"], b["Pa1"], sign, pair.zero, pair.tiny), excess=0.75)
        after = pair.read()
        deepest = min(deepest, OC.check_moments_of_mixed_signs(pair, before, after, pair.reference(), worst, f"{case[0]} apply {it}"))
        # each apply is compared on its own: what a cancellation left of mu is small against the rounding it was computed with,
        # so the oracle continues from the moments the kernel holds, not from its own
        for tx in ("critic", "actor"):
            pair.st.set_moments(tx, *({k: after[f"opt/{tx}/{m}"][k] for k in pair.sup[tx]} for m in ("mu", "nu")))
        before = after
    print(f"{case[0]} mixed signs: smallest |mu| / larger term {deepest:.2e}; {worst.text()}")
    assert deepest < 1e-2


# ---- 2. late counts and schedules -------------------------------------------------------------------------------------------------
def _one_full_step(pair, rng, scale=None, excess=0.75):
    """apply(7) with all three gradients injected; scale: {tx: global norm} for the critic's and the actor's gradient"""
    b = pair.b
    gc = OC.gradient(rng, 0, b["Pc"], pair.sign, pair.zero, pair.tiny)
    ga = OC.gradient(rng, b["Pa0"], b["Pa1"], pair.sign, pair.zero, pair.tiny)
    if scale is not None:
        gc = (gc.astype(np.float64) * (scale["critic"] / np.linalg.norm(gc.astype(np.float64)))).astype(np.float32)
        ga = (ga.astype(np.float64) * (scale["actor"] / np.linalg.norm(ga.astype(np.float64)))).astype(np.float32)
    before, ref_before = pair.read(), pair.reference()
    pair.apply(7, g_critic=gc, g_actor=ga, excess=excess)
    return before, ref_before, pair.read(), pair.reference(), gc, ga


@pytest.mark.parametrize("sid,count", OC.SCHEDULE_CASES, ids=[f"{s}-{c}" for s, c in OC.SCHEDULE_CASES])
def test_late_counts_and_schedules(gpu, sid, count):
    over = next(o for s, o, _ in OC.SCHEDULES if s == sid)
    pair = OC.Pair(OC.COUNT_CASE, cfg_override=over)
    pair.set_count(count)
    want_lr = {tx: np.float32(pair.st.lr_at(count, tx)) for tx in O.TX_NAMES}
    worst = OC.Worst()
    before, ref_before, after, ref_after, _, _ = _one_full_step(pair, np.random.default_rng(12))
    info = pair.core.read_info()
    for tx in O.TX_NAMES:
        got = np.float32(info[f"{tx}_lr"])
        print(f"{sid} count {count}: {tx}_lr {got!r}, lr_at {want_lr[tx]!r}, apart {abs(float(got) - float(want_lr[tx])) / float(np.spacing(want_lr[tx])):.2f} ulp")
        assert abs(float(got) - float(want_lr[tx])) <= float(np.spacing(want_lr[tx])), (tx, got, want_lr[tx])
        kw = pair.st.tx_opt(tx)
        if kw["cosine_decay_steps"] is not None and count >= max(kw["cosine_decay_steps"], kw["warmup_steps"] + 1):
            # at and beyond the end of the decay: exactly 0.0, and the leaves only this optimizer moves stay bit-identical
            assert float(want_lr[tx]) == 0.0 and int(_bits(got)[0]) == 0, (tx, got)
            only = [k for k in pair.sup[tx] if all(k not in pair.sup[o] for o in O.TX_NAMES if o != tx)]
            assert only
            for k in only:
                assert np.array_equal(_bits(before["params"][k]), _bits(after["params"][k])), (tx, k)
    OC.check_step(pair, before, after, ref_before, ref_after, 7, worst, f"{sid} count {count}")
    assert pair.core.step == pair.st.step == count + 1
    print(f"{sid} count {count}: {worst.text()}")


# (id, the global norm of the critic's / the actor's gradient and |g| of the temperature's, as multiples of each one's clip)
CLIP_CASES = [("half", 0.5, 0.5, 0.5), ("double", 2.0, 2.0, 2.0), ("1e6", 1e6, 1e6, 1e6), ("zero", 0.0, 0.0, 0.0),
              ("critic_binds_actor_free", 2.0, 0.5, 0.5), ("actor_binds_critic_free", 0.5, 2.0, 2.0)]
CLIP = {"critic": 0.5, "actor": 0.25, "temperature": 0.01}


@pytest.mark.parametrize("cid,mc,ma,mt", CLIP_CASES, ids=[c[0] for c in CLIP_CASES])
def test_clip_by_global_norm(gpu, cid, mc, ma, mt):
    """A clip that binds on one optimizer leaves the other's moments those of its unclipped gradient (the oracle's, within 2e-6):
    the critic's norm 2 x 0.5 and the actor's 0.5 x 0.25 differ by a factor 8, so a scale taken from the other optimizer's norm
    moves every moment it touches far outside the bound."""
    pair = OC.Pair(OC.COUNT_CASE, cfg_override=dict(opt={tx: {"clip_grad_norm": c} for tx, c in CLIP.items()}))
    rng = np.random.default_rng(13)
    lam = float(pair.st.params["temp/lagrange"])
    excess = mt * CLIP["temperature"] * (1.0 + np.exp(-lam))        # sigmoid(lam) * excess = mt x the clip
    worst = OC.Worst()
    scale = {"critic": mc * CLIP["critic"], "actor": ma * CLIP["actor"]}
    if mc == 0.0:
        pair.zero[:] = True
        scale = None
    before, ref_before, after, ref_after, gc, ga = _one_full_step(pair, rng, scale, excess)
    if scale is not None:
        for tx, g, m in (("critic", gc, mc), ("actor", ga, ma)):
            n = float(np.linalg.norm(g.astype(np.float64)))
            assert abs(n / CLIP[tx] - m) < 1e-3 * m, (tx, n)
    OC.check_step(pair, before, after, ref_before, ref_after, 7, worst, f"clip {cid}")
    print(f"clip {cid}: {worst.text()}")


# ---- 3. the deferred target-trunk EMA ---------------------------------------------------------------------------------------------
TRUNK_CFG = dict(OC.PIX, image_keys=("wrist",), S=3, A=3, hidden=64, ensemble=2)
PROBE = "trunk/norm_init/bias"      # the leaf the step-by-step twin reads after every apply


def _trunk_targets(trunk, seed=21):
    """target = online + noise: a leaf-sized scale on a third of the elements, one ulp on a third, nothing on a third"""
    rng = np.random.default_rng(seed)
    out = {}
    for k, p in trunk.items():
        p = np.asarray(p, np.float32)
        kind = rng.integers(0, 3, p.shape)
        big = (p + np.abs(p).max() * rng.standard_normal(p.shape)).astype(np.float32)
        one = np.nextafter(p, np.where(rng.random(p.shape) < 0.5, -np.inf, np.inf).astype(np.float32))
        out[k] = np.where(kind == 0, big, np.where(kind == 1, one, p)).astype(np.float32)
    return out


def _trunk_core(B=4):
    cfg = O.Config(**TRUNK_CFG)
    trunk, theta = O.init_params(cfg, 42)
    core = AH.load_leaves(AH.make_core(cfg, B), cfg, trunk, theta)
    t0 = _trunk_targets(trunk)
    core.load_flat("target_params", t0)
    core.debug_set("g_critic", np.zeros(4, np.float32))
    return cfg, core, trunk, t0


def _applies(core, n, read_each=False):
    """n critic applies with applies of the other two optimizers in between, which run no target update (sac.py:284-285)"""
    for i in range(n):
        core.apply(1)
        if i % 3 == 1:
            core.apply(6)
        if read_each:
            core.get("target_params", PROBE)


def _closed_form(p, t0, tau, n):
    p, t0 = np.asarray(p, np.float64), np.asarray(t0, np.float64)
    return p + (t0 - p) * (1.0 - tau) ** n


def _check_closed_form(what, got, ref, n, tau):
    """within min(n, 1 / tau) ulp of the leaf's largest element: each step rounds once and the recurrence contracts by 1 - tau"""
    worst = 0.0
    for k in ref:
        u = float(np.spacing(np.float32(np.abs(ref[k]).max())))
        e = float(np.abs(got[k].astype(np.float64) - ref[k].reshape(-1)).max()) / u
        worst = max(worst, e)
        assert e <= min(n, 1.0 / tau), (what, k, e, min(n, 1.0 / tau))
    return worst


@pytest.mark.parametrize("n", [1, 2, 7, 300])
def test_pending_trunk_ema_steps_equal_single_steps_and_the_closed_form(gpu, n):
    cfg, lazy, trunk, t0 = _trunk_core()
    _, eager, _, _ = _trunk_core()
    _applies(lazy, n)
    _applies(eager, n, read_each=True)
    got = {k: lazy.get("target_params", k) for k in trunk}
    step = {k: eager.get("target_params", k) for k in trunk}
    moved = 0
    for k in trunk:
        assert np.array_equal(_bits(got[k]), _bits(step[k])), (n, k, "one flush of n steps differs from n flushes of one step")
        moved += int(np.count_nonzero(_bits(got[k]) != _bits(t0[k].reshape(-1))))
        assert np.array_equal(_bits(lazy.get("params", k)), _bits(np.asarray(trunk[k], np.float32).reshape(-1))), (k, "online trunk moved")
    assert moved > sum(v.size for v in trunk.values()) // 4, "the target trunk did not move: nothing was observed"
    ref = {k: _closed_form(trunk[k], t0[k], cfg.tau, n) for k in trunk}
    w = _check_closed_form(f"n = {n}", got, ref, n, cfg.tau)
    print(f"trunk EMA n = {n}: worst distance from the fp64 closed form {w:.2f} ulp of the leaf's largest element (bound {min(n, 1 / cfg.tau):g}); "
          f"{moved} elements moved")
    assert lazy.step == eager.step == n + n // 3 + (1 if n % 3 == 2 else 0)
    # reading again applies nothing more
    for k in (PROBE, "trunk/conv_init"):
        assert np.array_equal(_bits(lazy.get("target_params", k)), _bits(got[k]))


def test_pending_steps_belong_to_the_online_values_they_were_counted_at(gpu):
    """serl_agent_set of an online trunk leaf flushes first: 2 steps towards the old values, then 3 towards the new"""
    cfg, core, trunk, t0 = _trunk_core()
    k = "trunk/block1/gn0/scale"
    new = (np.asarray(trunk[k], np.float32) + np.float32(0.5)).astype(np.float32)
    _applies(core, 2)
    core.set("params", k, new)
    _applies(core, 3)
    got = core.get("target_params", k)
    ref = _closed_form(new, _closed_form(trunk[k], t0[k], cfg.tau, 2), cfg.tau, 3)
    wrong = _closed_form(new, t0[k], cfg.tau, 5)
    u = float(np.spacing(np.float32(np.abs(ref).max())))
    assert np.abs(wrong - ref).max() > 1000 * u
    assert np.abs(got - ref).max() <= 5 * u, (np.abs(got - ref).max() / u, np.abs(got - wrong).max() / u)
    other = "trunk/block1/gn0/bias"     # every other leaf: five steps towards its unchanged values
    assert np.abs(core.get("target_params", other) - _closed_form(trunk[other], t0[other], cfg.tau, 5)).max() <= \
        5 * float(np.spacing(np.float32(np.abs(trunk[other]).max())))


def test_snapshot_and_checkpoint_carry_the_flushed_target_trunk(gpu, tmp_path):
    from serl_amd.agents.drq import DrQAgent
    from serl_amd.agents.snapshot import SnapshotHandle, section_mask
    from serl_amd.utils.checkpoint import restore_checkpoint, save_checkpoint
    n = 7
    cfg, core, trunk, t0 = _trunk_core()
    _, twin, _, _ = _trunk_core()
    _applies(core, n)
    _applies(twin, n, read_each=True)
    want = {k: twin.get("target_params", k) for k in trunk}
    h = SnapshotHandle(core, section_mask(("target_params",)), 1)
    try:
        slot = h.take()
        h.wait(slot)
        for k in trunk:
            assert np.array_equal(_bits(np.array(h.leaf(slot, "target_params", k, core))), _bits(want[k])), ("snapshot", k)
        h.release(slot)
    finally:
        h.close()
    for k in trunk:         # ... and the take consumed the pending steps: a read applies none of them again
        assert np.array_equal(_bits(core.get("target_params", k)), _bits(want[k])), ("after the snapshot", k)

    def agent():
        obs = {"image": np.zeros((1, 32, 32, 3), np.uint8), "state": np.zeros((1, 3), np.float32)}
        mlp = {"hidden_dims": [64, 64], "activations": "tanh", "use_layer_norm": True}
        return DrQAgent.create_drq(3, obs, np.zeros((1,), np.float32), encoder_type="resnet-pretrained", use_proprio=True,
                                   image_keys=("image",), critic_network_kwargs=mlp, policy_network_kwargs=dict(mlp),
                                   critic_ensemble_size=3, critic_subsample_size=2, batch_size=4)
    a, b = agent(), agent()
    for ag in (a, b):
        ag.core.load_flat("params", trunk)
        ag.core.load_flat("target_params", t0)
        ag.core.debug_set("g_critic", np.zeros(4, np.float32))
    _applies(a.core, n)
    _applies(b.core, n, read_each=True)
    path = save_checkpoint(str(tmp_path / "ckpt"), a, step=a.core.step)
    fresh = agent()
    restore_checkpoint(path, fresh)
    for k in trunk:
        w = b.core.get("target_params", k)
        assert np.array_equal(_bits(fresh.core.get("target_params", k)), _bits(w)), ("checkpoint", k)
        assert np.array_equal(_bits(w), _bits(want[k])), ("the two agents' trunks", k)
        assert np.array_equal(_bits(fresh.core.get("params", k)), _bits(np.asarray(trunk[k], np.float32).reshape(-1))), k


def test_update_high_utd_counts_one_trunk_step_per_minibatch(gpu):
    B, utd = 6, 3
    cfg = O.Config(**TRUNK_CFG)
    trunk, theta = O.init_params(cfg, 42)
    core = AH.load_leaves(AH.make_core(cfg, B), cfg, trunk, theta)
    # the critic reads the target trunk: keep it close to the online one (one ulp / nothing / 1e-3 of the leaf), the comparison is in ulp
    rng = np.random.default_rng(22)
    t0 = {}
    for k, p in trunk.items():
        kind = rng.integers(0, 3, p.shape)
        t0[k] = np.where(kind == 0, p + np.float32(1e-3) * np.abs(p).max() * rng.standard_normal(p.shape).astype(np.float32),
                         np.where(kind == 1, np.nextafter(p, np.float32(np.inf)), p)).astype(np.float32)
    core.load_flat("target_params", t0)
    b = AH.synth_batch(cfg, B, seed=23)
    noise = O.make_noise(cfg, B, seed=24, utd_ratio=utd)
    core.update_high_utd(AH.batch_to_device(cfg, b), utd, AH.noise_to_device(cfg, noise))
    assert core.step == utd + 1
    got = {k: core.get("target_params", k) for k in trunk}
    for n_wrong in (utd - 1, utd + 1):
        k = "trunk/conv_init"
        u = float(np.spacing(np.float32(np.abs(trunk[k]).max())))
        assert np.abs(_closed_form(trunk[k], t0[k], cfg.tau, n_wrong) - _closed_form(trunk[k], t0[k], cfg.tau, utd)).max() > 8 * u
    w = _check_closed_form("high_utd", got, {k: _closed_form(trunk[k], t0[k], cfg.tau, utd) for k in trunk}, utd, cfg.tau)
    print(f"update_high_utd(utd = 3): target trunk within {w:.2f} ulp of three EMA steps")


# ---- 4. the BC and classifier slices ----------------------------------------------------------------------------------------------
def _check_slice_step(what, count, lr, leaves, before, after, mu, nu):
    """the step of every trainable element from the READ-BACK moments: -lr (mu / bc1) / (sqrt(nu / bc2) + 1e-8), bc of count + 1"""
    t = count + 1
    bc1, bc2 = 1.0 - 0.9 ** t, 1.0 - 0.999 ** t
    lr = float(np.float32(lr))
    worst, moved = 0.0, 0
    for k in leaves:
        m, v = mu[k].astype(np.float64), nu[k].astype(np.float64)
        d_ref = -lr * (m / bc1) / (np.sqrt(v / bc2) + 1e-8)
        d_got = after[k].astype(np.float64) - before[k].astype(np.float64)
        err = np.abs(d_got - d_ref)
        bound = OC.STEP_REL * np.abs(d_ref) + 2.0 * np.maximum(OC.ulp(before[k]), OC.ulp(after[k]))
        i = int(np.argmax(err / bound))
        worst = max(worst, float(err[i] / bound[i]))
        moved += int(np.count_nonzero(d_got))
        assert err[i] <= bound[i], (what, count, k, i, d_got[i], d_ref[i], err[i], bound[i])
    assert moved, (what, "no parameter moved")
    print(f"{what} at count {count}: worst step err / bound {worst:.3f}, {moved} elements moved")


@pytest.mark.parametrize("count", [0, 999, 10 ** 6])
def test_bc_slice_step_at_late_counts(gpu, count):
    import bc_oracle as BO
    import learner_regimes as LR
    row = next(r for r in LR.BC_EDGES if r[0] == "B7")
    cfg, B = LR.bc_edge_cfg(row)
    trunk, theta = LR.bc_theta(cfg, "max_only")
    inp = LR.bc_inputs(cfg, B, "max_only")
    agent = LR.bc_agent(cfg, B, trunk, theta)
    agent.state._set_step(count)
    train, frozen = agent.leaves(trainable=True), agent.leaves(trainable=False)
    assert sorted(train) == sorted(AH.product_name(k, cfg.image_keys) for k in BO.TRAIN) and frozen
    for k in train:
        assert not agent.get("opt/mu", k).any() and not agent.get("opt/nu", k).any()
    before = {k: agent.get("params", k) for k in train + frozen}
    agent.update(LR.bc_batch(inp["frames"], inp["state"], inp["action"]), masks=inp["masks"])
    assert agent.state.step == count + 1
    after = {k: agent.get("params", k) for k in train + frozen}
    mu, nu = ({k: agent.get(sec, k) for k in train} for sec in ("opt/mu", "opt/nu"))
    _check_slice_step("bc", count, 3e-4, train, before, after, mu, nu)
    for k in frozen:
        assert np.array_equal(_bits(before[k]), _bits(after[k])), k


@pytest.mark.parametrize("count", [0, 999, 10 ** 6])
def test_classifier_slice_step_at_late_counts(gpu, count):
    import learner_regimes as LR
    from serl_amd.networks.reward_classifier import train_step
    keys, params, frames, labels, masks = LR.cls_edge(next(r for r in LR.CLS_EDGES if r[0] == "B7"))
    lr = 1e-4
    c = LR.classifier(keys, LR.EDGE_HW, LR.EDGE_HW, params, len(labels), lr)
    c._set_step(count)
    frozen = [k for k in c._counts if k.startswith("trunk/")]
    train = [k for k in c._counts if not k.startswith("trunk/")]
    assert frozen and train
    for k in train:
        assert not c._get("opt/mu", k).any() and not c._get("opt/nu", k).any()
    before = {k: c.get(k) for k in train + frozen}
    c, _, _ = train_step(c, {"data": frames, "labels": labels.reshape(-1, 1)}, None,
                         masks={k: np.asarray(m, np.uint8) for k, m in masks.items()})
    assert c.step == count + 1
    after = {k: c.get(k) for k in train + frozen}
    mu, nu = ({k: c._get(sec, k) for k in train} for sec in ("opt/mu", "opt/nu"))
    _check_slice_step("classifier", count, lr, train, before, after, mu, nu)
    for k in frozen:
        assert np.array_equal(_bits(before[k]), _bits(after[k])), k
        assert not c._get("opt/mu", k).any() and not c._get("opt/nu", k).any()
