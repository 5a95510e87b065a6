"""CPU: what the layout table of tests/optimizer_cases.py covers, proved on the oracle's trainable_param_shapes alone.

adam_ema_kernel (serl_amd/csrc/heads.hip) hands a 4-vector to its 16-byte fast path or to adam_elem depending on where the vector
lies relative to Pc, Pa0, Pa1 and P - 1; tests/test_optimizer_layouts_gpu.py checks every element of every layout, and this file
makes sure the layouts put the four boundaries at every residue mod 4, with a straddling vector each, in both orders of Pa0 and
Pc.  Each property is asserted on its own, so a table that loses one says which."""
import numpy as np
import pytest

from oracle import drq_oracle as O
import agent_helpers as AH
import optimizer_cases as OC


def _all():
    return {c[0]: OC.boundaries(OC.layout_shapes(c)) for c in OC.LAYOUTS}


def test_the_boundaries_are_the_ones_the_agent_tests_derive():
    """Pc, Pa0, Pa1 as test_agent_gpu.py::test_adam_ema_injected / _check_grads take them from AH.leaf_slices, for every layout
    whose leaves are the oracle's own (the uniform policy's are not: its Pa1 ends at actor/log_stds)"""
    for c in OC.LAYOUTS:
        cfg, akw = OC.layout_config(c)
        if akw.get("std_parameterization") == "uniform":
            continue
        sl, P = AH.leaf_slices(cfg)
        b = OC.boundaries(OC.layout_shapes(c))
        assert b["Pc"] == sl.get("enc/proprio/ln/bias", sl["critic/head/bias"])[1], c[0]
        assert b["Pa0"] == sl.get("enc/proprio/dense/kernel", sl["actor/w1"])[0], c[0]
        assert b["Pa1"] == sl["actor/logstd/bias"][1] and b["P-1"] == P - 1 == sl["temp/lagrange"][0], c[0]


@pytest.mark.parametrize("boundary", OC.BOUNDARIES)
def test_every_boundary_takes_every_residue_mod_4(boundary):
    have = {b[boundary] % 4: name for name, b in _all().items()}
    missing = sorted(set(range(4)) - set(have))
    assert not missing, f"{boundary} never lies at residue(s) {missing} mod 4 in optimizer_cases.LAYOUTS (has {have})"


@pytest.mark.parametrize("boundary", OC.BOUNDARIES)
def test_every_boundary_has_a_straddling_vector(boundary):
    hits = []
    for c in OC.LAYOUTS:
        v = OC.boundary_vectors(OC.layout_shapes(c)).get(boundary)
        if v is not None:
            x = OC.boundaries(OC.layout_shapes(c))[boundary]
            assert v[0] % 4 == 0 and v[0] < x <= v[-1] and len(v) <= 4, (c[0], boundary, x, v)
            hits.append(c[0])
    assert hits, f"no layout has a 4-vector that straddles {boundary}"


def test_a_layout_has_the_actor_support_start_inside_the_critic_support():
    """the proprio encoder, which both optimizers update"""
    hits = [n for n, b in _all().items() if b["Pa0"] < b["Pc"]]
    assert hits, "no layout with Pa0 < Pc"
    for c in OC.LAYOUTS:
        if c[0] in hits:
            sup = OC.support(OC.layout_shapes(c))
            both = set(sup["critic"]) & set(sup["actor"])
            assert both == {f"enc/proprio/{k}" for k in ("dense/kernel", "dense/bias", "ln/scale", "ln/bias")}, (c[0], both)


def test_a_layout_has_the_two_supports_adjacent():
    """a state-only agent"""
    hits = [n for n, b in _all().items() if b["Pa0"] == b["Pc"]]
    assert hits, "no layout with Pa0 == Pc"


def test_the_table_holds_the_kinds_the_issue_lists():
    kinds = {}
    for c in OC.LAYOUTS:
        cfg, akw = OC.layout_config(c)
        kinds.setdefault("state" if cfg.state_only else ("small" if cfg.small else "drq"), []).append((cfg, akw))
    assert {c.hidden for c, _ in kinds["state"]} >= {64, 192, 320} and {c.A for c, _ in kinds["state"]} >= {1, 4, 5, 7}
    assert {c.n_cam for c, _ in kinds["drq"]} == {1, 2, 3}
    assert {c.S for c, _ in kinds["drq"]} >= {1, 3, 5} and {c.A for c, _ in kinds["drq"]} >= {3, 6, 33}
    assert all((c.H, c.W) == (32, 32) for c, _ in kinds["drq"] + kinds["small"])
    assert any(a.get("std_parameterization") == "uniform" for _, a in kinds["state"])
    wd = [c for c, _ in kinds["state"] if c.opt]
    assert wd and all(wd[0].opt[tx].get("weight_decay") for tx in O.TX_NAMES)
    # the SmallEncoder's conv leaves lie inside the critic optimizer's support and outside the actor's
    small = next(c for c in OC.LAYOUTS if OC.layout_config(c)[0].small)
    sup = OC.support(OC.layout_shapes(small))
    convs = [k for k in OC.layout_shapes(small) if "/conv" in k]
    assert convs and set(convs) <= set(sup["critic"]) and not set(convs) & set(sup["actor"])


def test_the_supports_partition_as_the_kernel_assumes():
    """every leaf ends inside or outside each support (no leaf straddles Pc, Pa0 or Pa1), the temperature is the last leaf, and
    every leaf belongs to at least one optimizer"""
    for c in OC.LAYOUTS:
        sh = OC.layout_shapes(c)
        sl, P = OC.slices_of(sh)
        b, sup = OC.boundaries(sh), OC.support(sh)
        assert list(sl)[-1] == "temp/lagrange" and sl["temp/lagrange"] == (P - 1, P) and b["Pa1"] == P - 1
        for k, (lo, hi) in sl.items():
            for x in (b["Pc"], b["Pa0"], b["Pa1"]):
                assert not lo < x < hi, (c[0], k, x)
            assert sum(k in sup[tx] for tx in O.TX_NAMES) >= 1, (c[0], k)


def test_the_inputs_hold_what_the_bounds_assume():
    """per leaf of four elements or more: exact zeros and 1e-20 entries in every gradient; a preset nu is zero only where mu and
    the gradients are; gradients and mu share the element's sign; |g| spans 1e-9 .. 1e3"""
    P = 5000
    sign, (zero, tiny) = OC.sign_pattern(P), OC.zero_pattern(P)
    rng = np.random.default_rng(0)
    g = OC.gradient(rng, 100, P, sign, zero, tiny)
    mu, nu = OC.preset_moments(rng, 100, P, sign, zero)
    assert (g[zero[100:]] == 0).all() and zero[100:].sum() > 10 and (np.abs(g[tiny[100:]]) == np.float32(1e-20)).all()
    assert np.float32(1e-20) * np.float32(1e-20) < np.finfo(np.float32).tiny
    reg = ~(zero[100:] | tiny[100:])
    assert np.abs(g[reg]).min() >= 9.9e-10 and np.abs(g[reg]).max() <= 1.01e3 and np.abs(g[reg]).min() < 1e-8 < 1e2 < np.abs(g[reg]).max()
    assert (g * sign[100:] >= 0).all() and (mu * sign[100:] >= 0).all() and (nu >= 0).all()
    assert ((nu == 0) == (mu == 0)).all() and (nu == 0).any() and (g[nu == 0] == 0).all()


def test_schedule_tables_reach_the_counts_the_issue_lists():
    assert OC.COUNTS == [0, 1, 2, 9, 999, 1999, 2000, 2001, 99_999, 1_000_000, 2 ** 24 + 1]
    assert OC.COSINE_COUNTS == [99, 100, 101, 550, 999, 1000, 1001, 10 ** 6]
    st = O.TrainState(O.Config(**dict(OC.COUNT_CASE[1], opt={tx: dict(OC.COSINE) for tx in O.TX_NAMES})), {}, {})
    assert st.lr_at(1000) == 0.0 and st.lr_at(10 ** 6) == 0.0 and st.lr_at(999) > 0.0 and st.lr_at(100) == 1e-3
    # cosine_decay_steps <= warmup_steps: T clamps to 1
    over = dict(OC.SCHEDULES[2][1])
    st = O.TrainState(O.Config(**dict(OC.COUNT_CASE[1], **over)), {}, {})
    for tx in O.TX_NAMES:
        assert st.tx_opt(tx)["cosine_decay_steps"] <= st.tx_opt(tx)["warmup_steps"]
        assert st.lr_at(50, tx) == st.cfg.lr and st.lr_at(51, tx) == 0.0 and st.lr_at(49, tx) == st.cfg.lr * 49 / 50


def test_set_count_moves_step_and_the_three_counts_together():
    cfg = O.Config(**OC.COUNT_CASE[1])
    st = O.TrainState(cfg, *O.init_params(cfg, 1))
    st.set_count(999)
    assert st.step == 999 and all(st.opt[tx]["count"] == 999 for tx in O.TX_NAMES)
    O.apply_gradients(st, {})
    assert st.step == 1000 and all(st.opt[tx]["count"] == 1000 for tx in O.TX_NAMES)


# ---- the comparator itself: a NaN from the kernel must not pass ---------------------------------------------------------------------
def test_worst_add_flags_nan_inf_and_excess_and_nothing_else():
    w = OC.Worst()
    assert w.add("q", [0.0, 5e-7, 1e-9], [1e-6] * 3) is None
    assert w.add("q", [0.0, 0.0], [0.0, 0.0]) is None                     # exact zeros against a zero bound hold
    assert w.add("q", [0.0, np.nan, 1e-9], [1e-6] * 3) == 1
    assert w.add("q", [0.0, 1e-9, np.inf], [1e-6] * 3) == 2
    assert w.add("q", [0.0, 2e-6, 1e-9], [1e-6] * 3) == 1
    assert w.add("q", [1e-30], [0.0]) == 0                                # anything against a zero bound does not
    assert w.add("q", [1e-9], [np.nan]) == 0
    assert w.v["q"][0] == np.inf
    w2 = OC.Worst()
    w2.add("r", [1e-9], [1e-6], raw=[np.nan])
    assert w2.v["r"] == (1e-3, np.inf)


def _host_pair(case):
    """what check_step needs of a Pair, without a device: the oracle's state before and after one critic step, and its float32
    rounding standing in for the kernel's read-back"""
    from types import SimpleNamespace
    cfg, _ = OC.layout_config(case)
    shapes = OC.layout_shapes(case)
    sl, P = OC.slices_of(shapes)
    pair = SimpleNamespace(cfg=cfg, shapes=shapes, sl=sl, P=P, b=OC.boundaries(shapes), sup=OC.support(shapes))
    trunk, theta = OC.layout_theta(case, 42)
    st = O.TrainState(cfg, trunk, theta)
    st.target = O.to_torch(OC.layout_theta(case, 43)[1], st.dtype)
    pair.st = st
    ref = lambda: OC.Pair.reference(pair)                                             # noqa: E731
    f32 = lambda r: {sec: {k: v.astype(np.float32) for k, v in d.items()} for sec, d in r.items()}   # noqa: E731
    before = f32(ref())
    ref_before = {sec: {k: v.astype(np.float64) for k, v in d.items()} for sec, d in before.items()}
    sign, (zero, tiny) = OC.sign_pattern(P), OC.zero_pattern(P)
    # (no 1e-20 entries: from zero moments their squares are float32 denormals, which the rounding that stands in for the kernel
    #  does not keep to 3e-5; Pair presets a positive nu wherever a gradient is 1e-20)
    g = OC.gradient(np.random.default_rng(1), 0, pair.b["Pc"], sign, zero, np.zeros_like(tiny))
    O.apply_gradients(st, {"critic": OC.Pair._tree(pair, g, "critic", 0)})
    O.target_update(st)
    ref_after = ref()
    return pair, before, f32(ref_after), ref_before, ref_after


def test_check_step_passes_the_rounded_oracle_and_refuses_a_nan_anywhere():
    case = next(c for c in OC.LAYOUTS if c[0] == "state_w64_A1_S3_E3")
    pair, before, after, ref_before, ref_after = _host_pair(case)
    OC.check_step(pair, before, after, ref_before, ref_after, 1, OC.Worst(), "host")
    vec = OC.boundary_vectors(pair.shapes)["Pc"]
    leaf = next(k for k, (lo, hi) in pair.sl.items() if lo <= vec[0] < hi)
    for sec, bad in (("opt/critic/mu", np.nan), ("opt/critic/nu", np.nan), ("params", np.nan), ("target_params", np.nan),
                     ("params", np.inf), ("opt/critic/mu", 1.0)):
        poisoned = {s: dict(d) for s, d in after.items()}
        a = poisoned[sec][leaf].copy()
        a[vec[0] - pair.sl[leaf][0]] = bad
        poisoned[sec][leaf] = a
        with pytest.raises(AssertionError, match="straddling Pc"):
            OC.check_step(pair, before, poisoned, ref_before, ref_after, 1, OC.Worst(), f"{sec} <- {bad}")
    poisoned = {s: dict(d) for s, d in after.items()}       # a NaN outside an optimizer's support
    a = poisoned["opt/actor/mu"][leaf].copy()
    a[0] = np.nan
    poisoned["opt/actor/mu"][leaf] = a
    with pytest.raises(AssertionError, match="outside the support"):
        OC.check_step(pair, before, poisoned, ref_before, ref_after, 1, OC.Worst(), "outside")
