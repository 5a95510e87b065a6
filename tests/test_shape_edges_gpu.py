"""GPU parity at image sizes and dimensions that are not powers of two (tests/shape_edges.py; what the table covers is proved
in test_shape_edges_cpu.py): the frozen trunk in both arithmetic modes with the path each case takes asserted from the
library's own plan, the update chain at tile tails and limits, the classifier and the replay crop at 84-pixel extents.
Bounds are the suite's: 5e-6 of the fp64 oracle for trunk features and 2e-6 between fused and separate variants of one pass
(test_agent_gpu.py::test_trunk_forward, ::test_fused_projection), 1e-4 for update quantities (TOL)."""
import itertools

import numpy as np
import pytest
import torch

from oracle import drq_oracle as O
import agent_helpers as AH
import shape_edges as SE
from test_agent_gpu import MODES, TOL, _compare_state

pytestmark = pytest.mark.gpu


# ---- frozen trunk ------------------------------------------------------------------------------------------------------------
def _assert_plan(plan, H, W, n):
    """The split-fp16 pass took the path this size was put in the table for (serl_agent_trunk_plan)."""
    gh, gw = SE.geometry(H, W)
    assert plan["images"] == n, plan
    fused_pool = gh["conv_init_out"] % 16 == 0 and gw["conv_init_out"] % 16 == 0
    assert plan["pool"] == ((2 if n % 512 == 0 else 1) if fused_pool else 0), plan
    want = SE.expected_pads(H, W)
    for layer, pads in want.items():
        kern, cfg, pmode, _, got = plan[layer]
        i = int(layer[1])
        P = gh["stage_out"][i] * gw["stage_out"][i]
        if kern == "F":      # the projection rode on conv0's launch: only where conv0's tap (0, 0) is the projection's pixel
            conv0 = plan[layer.replace("proj", "conv0")]
            assert layer.endswith("proj") and conv0[0] == "D" and conv0[4] == (0, 0) == want[layer.replace("proj", "conv0")], (layer, plan)
            assert (cfg, pmode, got) == (conv0[1], conv0[2], (0, 0)) and pmode != 3, (layer, plan)
            continue
        assert got == pads, (layer, got, pads, plan)           # the library's SAME pad is XLA's
        # statistics mode, restated from the rule: 0 = a wave's rows (32 on the 64x64 tile, else 64) lie in one image, 1 / 2 = images
        # of 32 / 16 pixels (1 only on tiles whose waves hold 64 rows and not on the LDS-DMA kernel's 128x64 tile), 3 = none of
        # these: waves straddle images and the statistics come from the separate kernel
        wave_rows = 32 if cfg == 2 else 64
        mode = 0 if P % wave_rows == 0 else (1 if P == 32 else (2 if P == 16 else 3))
        if mode == 1 and (cfg == 2 or (kern == "D" and cfg == 4)):
            mode = 3
        assert pmode == mode, (layer, P, cfg, pmode, mode, plan)
    if not fused_pool or gw["pool_out"] not in (32, 16):
        assert all(plan[f"b{i}_conv{k}"][0] != "S" for i in range(4) for k in (0, 1)), plan   # no row-slab kernel off 32 / 16 columns


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("H,W", SE.SIZES)
def test_trunk_forward_at_sizes_off_the_powers_of_two(gpu, H, W, mode):
    cfg = O.Config(image_keys=("a",), H=H, W=W, S=4, A=2)
    st, core = AH.make_pair(cfg, B=4, trunk_mode=mode)
    rng = np.random.default_rng(H * 1000 + W)
    for n in (3, 7):          # 7 x (last-stage pixels) is no multiple of 64 for any size of the table but 32x32 (7 rows)
        img = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
        ref = O.trunk_forward(st.trunk, torch.tensor(img), torch.float64).numpy()
        got = core.trunk_forward(torch.tensor(img, device="cuda")).cpu().numpy()
        assert got.shape == ref.shape and ref.shape[1] * ref.shape[2] == SE.feat_hw(H, W)
        err = AH.rel_err(got, ref)
        print(f"trunk {mode} {H}x{W} n={n}: rel err vs fp64 = {err:.2e}")
        assert err < 5e-6, (n, err)
        if mode == "f16x3":
            _assert_plan(core.trunk_plan(), H, W, n)


@pytest.mark.parametrize("n", [1024, 128])
@pytest.mark.parametrize("H", [84, 96])
def test_trunk_full_batch_and_per_rank_kernels_at_84_and_96(gpu, H, n, monkeypatch):
    """Full-batch (1024 images) and per-rank (128) kernel selection where no tile is image-aligned: 84 -> maps of 21, 11, 6, 3
    pixels (stride-2 pads of 1 in stages 1 and 2, separate pooling), 96 -> 24, 12, 6, 3 (fused pooling, no row-slab kernel).
    GroupNorm is per image, so the first and last six images against the oracle are a complete check of those images; the whole
    output against the same pass with separate GroupNorm epilogues (SERL_GN_FUSE=0) and separate projection launches
    (SERL_PROJ_FUSE=0)."""
    cfg = O.Config(image_keys=("a",), H=H, W=H, S=4, A=2)
    st, core = AH.make_pair(cfg, B=n // 2, trunk_mode="f16x3")
    img = torch.randint(0, 256, (n, H, H, 3), dtype=torch.uint8, device="cuda", generator=torch.Generator("cuda").manual_seed(H))
    out = core.trunk_forward(img).clone()
    plan = core.trunk_plan()
    print(f"trunk {H}x{H} n={n}: plan {plan}")
    _assert_plan(plan, H, H, n)
    if n == 1024:
        for i, k in itertools.product((1, 2, 3), (0, 1)):
            assert plan[f"b{i}_conv{k}"][0] == "D", plan
        assert all(plan[f"b{i}_proj"][0] in ("D", "F") for i in (1, 2, 3)), plan
    if H == 84:
        assert plan["b1_proj"][0] != "F" and plan["b2_proj"][0] != "F", plan    # stride-2 pad 1: tap (0, 0) is not the projection's pixel
    scale = float(out.abs().max())
    for var in ("SERL_GN_FUSE", "SERL_PROJ_FUSE"):
        monkeypatch.setenv(var, "0")
        other = core.trunk_forward(img).clone()
        _assert_plan(core.trunk_plan(), H, H, n)
        monkeypatch.delenv(var)
        d = float((other - out).abs().max()) / scale
        print(f"trunk {H}x{H} n={n}: {var}=0 differs by {d:.2e}")
        assert d < 2e-6, (var, d)
    sel = list(range(6)) + list(range(n - 6, n))
    ref = O.trunk_forward(st.trunk, img[sel].cpu(), torch.float64).numpy()
    err = AH.rel_err(out[sel].cpu().numpy(), ref)
    print(f"trunk {H}x{H} n={n}: rel err vs fp64 = {err:.2e}")
    assert err < 5e-6, err


# ---- update chain ------------------------------------------------------------------------------------------------------------
class _Figures:
    """every figure of a case is printed before the first assertion fails, so one run shows all of them"""

    def __init__(self, what):
        self.what, self.bad = what, []

    def add(self, name, err, tol=TOL):
        print(f"{self.what}: {name} = {err:.2e}")
        if not err < tol:
            self.bad.append((name, err))

    def check(self):
        assert not self.bad, (self.what, self.bad)


def _grads(fig, cfg, core, grads, tap):
    sl, _ = AH.leaf_slices(cfg)
    pc = sl.get("enc/proprio/ln/bias", sl["critic/head/bias"])[1]
    lo0 = 0 if tap == "g_critic" else sl.get("enc/proprio/dense/kernel", sl["actor/w1"])[0]
    g = core.debug(tap, {"g_critic": pc, "g_actor": sl["actor/logstd/bias"][1] - lo0}[tap])
    for k, gv in grads.items():
        lo, hi = sl[k]
        fig.add(f"{tap} {k}", AH.rel_err(g[lo - lo0:hi - lo0], gv.numpy().reshape(-1)))


def _info(fig, got, info, names):
    for k in names:
        fig.add(f"info {k}", abs(got[k] - info[k]) / max(1.0, abs(info[k])))


_IDS = [c[0] for c in SE.UPDATE_CASES]
_FROZEN = [c for c in SE.UPDATE_CASES if c[2] == "resnet-pretrained"]


def _critics(case, mode):
    cfg, B, _ = SE.update_config(case)
    st, core = AH.make_pair(cfg, B, trunk_mode=mode)
    b = AH.synth_batch(cfg, B, seed=3)
    noise = O.make_noise(cfg, B, seed=7)
    info, aux = O.update_critics(st, AH.batch_to_torch(b, torch.float64), O.noise_to_torch(noise, torch.float64))
    core.update_critics(AH.batch_to_device(cfg, b), AH.noise_to_device(cfg, noise))
    fig = _Figures(f"update_critics {case[0]} {mode or ''}")
    _info(fig, core.read_info(), info, ("critic_loss", "predicted_qs", "target_qs"))
    fig.add("q", AH.rel_err(core.debug("q", cfg.ensemble * B).reshape(cfg.ensemble, B), aux["q"].numpy()))
    fig.add("target_q", AH.rel_err(core.debug("target_q", B), aux["target_q"].numpy()))
    fig.add("next logp", AH.rel_err(core.debug("logp", B), aux["next_logp"].numpy()))
    _grads(fig, cfg, core, aux["grads"], "g_critic")
    fig.check()
    _compare_state(cfg, st, core)
    assert core.step == st.step == 1
    assert core.debug("ctr_nonzero", 1)[0] == 0


@pytest.mark.parametrize("case", SE.UPDATE_CASES, ids=_IDS)
def test_update_critics_at_edge_dimensions(gpu, case):
    _critics(case, None)


@pytest.mark.parametrize("case", _FROZEN, ids=[c[0] for c in _FROZEN])
def test_update_critics_at_edge_dimensions_exact_fp32_trunk(gpu, case):
    _critics(case, "f32")


# utd 1 for every row, and the row's own utd > 1 (B % utd == 0) where B has one: B = 1 has none
_UTD = [(c, 1) for c in SE.UPDATE_CASES] + [(c, c[10]) for c in SE.UPDATE_CASES if c[10] > 1]


@pytest.mark.parametrize("case,utd", _UTD, ids=[f"{c[0]}-utd{u}" for c, u in _UTD])
def test_update_high_utd_at_edge_dimensions(gpu, case, utd):
    cfg, B, _ = SE.update_config(case)
    st, core = AH.make_pair(cfg, B)
    b = AH.synth_batch(cfg, B, seed=4)
    noise = O.make_noise(cfg, B, seed=8, utd_ratio=utd)
    info, aux = O.update_high_utd(st, AH.batch_to_torch(b, torch.float64), O.noise_to_torch(noise, torch.float64), utd)
    core.update_high_utd(AH.batch_to_device(cfg, b), utd, AH.noise_to_device(cfg, noise))
    fig = _Figures(f"update_high_utd({utd}) {case[0]}")
    _info(fig, core.read_info(), info, ("critic_loss", "predicted_qs", "target_qs", "actor_loss", "temperature", "entropy", "temperature_loss"))
    _grads(fig, cfg, core, aux["g_actor"], "g_actor")
    fig.check()
    _compare_state(cfg, st, core, steps=utd + 1)
    assert core.step == st.step == utd + 1
    assert core.debug("ctr_nonzero", 1)[0] == 0


@pytest.mark.parametrize("case", SE.UPDATE_CASES, ids=_IDS)
def test_sample_actions_at_edge_dimensions(gpu, case):
    cfg, B, _ = SE.update_config(case)
    st, core = AH.make_pair(cfg, B)
    b = AH.synth_batch(cfg, B, seed=6)
    frames = torch.tensor(np.stack([b["obs"][k] for k in cfg.image_keys]), device="cuda") if cfg.image_keys else None
    state = torch.tensor(b["state"], device="cuda")
    feats = O.features(st, {k: torch.tensor(v) for k, v in b["obs"].items()})
    enc = O.encode(st.params, cfg, feats, torch.tensor(b["state"], dtype=torch.float64))
    mean, std = O.policy_head(st.params, cfg, enc)
    fig = _Figures(f"sample_actions {case[0]}")
    fig.add("mode", AH.rel_err(core.sample_actions(frames, state, None).cpu().numpy(), torch.tanh(mean).numpy()))
    eps = np.random.default_rng(0).standard_normal((B, cfg.A)).astype(np.float32)
    a, _ = O.sample_and_log_prob(mean, std, torch.tensor(eps, dtype=torch.float64))
    fig.add("sample", AH.rel_err(core.sample_actions(frames, state, torch.tensor(eps, device="cuda")).cpu().numpy(), a.numpy()))
    fig.check()
    assert core.debug("ctr_nonzero", 1)[0] == 0


@pytest.mark.parametrize("chain_fuse", ["1", "0"])
def test_draws_inside_the_kernels_equal_the_materialised_draws_at_odd_rows_and_columns(gpu, monkeypatch, chain_fuse):
    """test_drq_agent_gpu.py::test_draws_inside_the_kernels_equal_the_materialised_draws at B = 65 rows (minibatches of 13) and
    A = 33 columns on frames 84 high and 96 wide (the packed batch is cropped by the replay kernel, whose rows are whole
    16-byte vectors: W * 3 % 16 == 0): the in-kernel jax.random draws index rows and columns that are no multiple of any vector
    width.  Same keys, same elements: info, parameters and the key chain agree to the bit with the one-launch fill."""
    from serl_amd.utils.launcher import make_drq_agent
    monkeypatch.setenv("SERL_CHAIN_FUSE", chain_fuse)
    keys_, H, W, S, A, B = ("wrist",), 84, 96, 17, 33, 65
    obs0 = {k: np.zeros((1, H, W, 3), np.uint8) for k in keys_}
    obs0["state"] = np.zeros((1, S), np.float32)
    rng = np.random.default_rng(0)

    def batch():
        t = lambda a: torch.tensor(a, device="cuda")  # noqa: E731
        obs = {k: t(rng.integers(0, 256, (B, 2, H, W, 3), dtype=np.uint8)) for k in keys_}
        obs["state"] = t(rng.standard_normal((B, 1, S)).astype(np.float32))
        return {"observations": obs, "next_observations": {"state": t(rng.standard_normal((B, 1, S)).astype(np.float32))},
                "actions": t(rng.uniform(-1, 1, (B, A)).astype(np.float32)), "rewards": t((rng.random(B) < 0.3).astype(np.float32)),
                "masks": t((rng.random(B) < 0.9).astype(np.float32))}

    batches = [batch() for _ in range(3)]
    out = []
    for form in ("keys", "tensors"):
        agent = make_drq_agent(5, obs0, np.zeros((A,), np.float32), image_keys=keys_, encoder_type="resnet-pretrained", batch_size=B)
        agent.noise_form = form
        infos = []
        agent, info = agent.update_critics(batches[0]); infos.append(dict(info["critic"]))
        agent, info = agent.update_high_utd(batches[1], utd_ratio=5); infos.append({**info["critic"], **info["actor"], **info["temperature"]})
        agent, info = agent.update(batches[2]); infos.append({**info["critic"], **info["actor"], **info["temperature"]})
        torch.cuda.synchronize()
        assert agent.core.debug("ctr_nonzero", 1)[0] == 0
        out.append((infos, {k: agent.core.get("params", k) for k in ("critic/w1", "actor/w2", "actor/mean/kernel", "enc/0/dense/kernel", "enc/0/sle", "temp/lagrange")},
                    [int(v) for v in agent.state.rng]))
    assert out[0][0] == out[1][0], (out[0][0], out[1][0])
    assert out[0][2] == out[1][2]
    for k in out[0][1]:
        assert np.array_equal(out[0][1][k].view(np.uint32), out[1][1][k].view(np.uint32)), k


# ---- the classifier: same trunk, same camera heads ------------------------------------------------------------------------------
@pytest.mark.parametrize("keys,H,W,B", [(("front", "wrist"), 84, 84, 6), (("wrist",), 33, 47, 7)])
def test_classifier_logits_and_one_step_off_the_powers_of_two(gpu, keys, H, W, B):
    """test_classifier_train_gpu.py::test_one_step_at_the_timed_shape_equals_the_fp64_restatement at 84x84 (3x3 feature map)
    and 33x47 (2x2, max-pool with a padded top row), plus the inference logits."""
    import classifier_train_oracle as CT
    from oracle import classifier_oracle as CO
    from serl_amd.networks.reward_classifier import Classifier, train_step
    params = CO.make_params(keys, H, W, 31)
    rng = np.random.default_rng(32)
    frames = {k: rng.integers(0, 256, (B, 1, H, W, 3), dtype=np.uint8) for k in keys}
    masks = {k: rng.random((B, 4096)) < 0.9 for k in keys}
    masks["head"] = rng.random((B, 256)) < 0.9
    labels = (np.arange(B) < (B + 1) // 2).astype(np.float32)[:, None]
    st = CT.State(params, keys)
    feats = CT.features(params, keys, {k: v[:, 0] for k, v in frames.items()})
    th = {k: torch.tensor(np.asarray(v), dtype=torch.float64) for k, v in params.items()}
    c = Classifier(keys, H, W, max_batch=B, trainable=True, learning_rate=1e-4).load_flat(params)
    logits = c.apply_fn({"params": c.params}, frames)
    ref_logits = CT.forward(th, keys, feats).numpy()
    print(f"classifier {H}x{W}: max |logit - fp64| = {np.abs(logits - ref_logits).max():.2e}")
    assert logits.shape == (B, 1) and np.abs(logits - ref_logits).max() < 1e-4
    loss_ref, acc_ref, ev, grads = CT.train_step(st, feats, labels, masks)
    c, loss, acc = train_step(c, {"data": frames, "labels": labels}, None, masks={k: m.astype(np.uint8) for k, m in masks.items()})
    loss, acc = float(loss), float(acc)
    print(f"classifier {H}x{W} B={B}: loss {loss:.6f} (fp64 {loss_ref:.6f}), accuracy {acc} ({acc_ref}), min |eval logit| {np.abs(ev).min():.2e}")
    assert abs(loss - loss_ref) < 1e-4 * abs(loss_ref)
    assert np.float32(acc) == np.float32(acc_ref)
    for leaf, g in grads.items():   # the step-1 moments are the gradient: mu = 0.1 g, nu = 0.001 g^2
        name = f"enc/{keys.index(leaf.split('/')[1])}/{leaf.split('/', 2)[2]}" if leaf.startswith("enc/") else leaf
        mu, nu = c._get("opt/mu", name).astype(np.float64), c._get("opt/nu", name).astype(np.float64)
        assert np.abs(mu - 0.1 * g).max() <= 1e-4 * np.abs(0.1 * g).max() + 1e-30, leaf
        assert np.abs(nu - 0.001 * g * g).max() <= 1e-4 * np.abs(0.001 * g * g).max() + 1e-30, leaf


# ---- replay -> crop -> update at H = 84, W = 96 ---------------------------------------------------------------------------------
def test_replay_crop_update_at_84x96(gpu):
    """The buffer stores rows of whole 16-byte vectors (W * 3 % 16 == 0), H is free: gather + random shift byte-exact against
    the oracle's crop as test_replay_gpu.py::test_fused_gather_crop_matches_oracle does for the golden shapes, then one
    update_critics on the cropped batch against the fp64 oracle."""
    from helpers import make_spaces
    from oracle.replay_oracle import ReplayOracle, random_shift
    from serl_amd.agents.batch import DeviceBatch
    from serl_amd.data.data_store import MemoryEfficientReplayBufferDataStore, gather_crop
    from serl_amd.utils.synthetic import transition_stream
    keys, H, W, S, A, cap, B = ("front", "wrist"), 84, 96, 5, 3, 40, 6
    osp, asp = make_spaces(keys, H, W, 3, 1, S, A)
    rb = MemoryEfficientReplayBufferDataStore(osp, asp, cap, image_keys=keys)
    o = ReplayOracle(keys, H, W, 3, 1, S, A, cap)
    rb.seed(11), o.seed(11)
    for tr in itertools.islice(transition_stream(keys, H, W, 3, 1, S, A, 9, 5), 30):
        rb.insert(tr)
        o.insert(tr)
    rng = np.random.default_rng(7)
    for trial in range(3):
        idx = rb.sample_indices(B)
        assert (idx == o.sample_indices(B)).all()
        co = rng.integers(0, 9, size=(B, 2)).astype(np.int32)
        cn = rng.integers(0, 9, size=(B, 2)).astype(np.int32)
        if trial == 0:
            co[:], cn[:] = 0, 8
        out = DeviceBatch(B, len(keys), H, W, 3, S, A, 0)
        gather_crop([(rb, idx)], co, cn, out)
        torch.cuda.synchronize()
        ob = o.gather(idx)
        fr = out.frames.cpu().numpy()
        for c, k in enumerate(keys):
            packed = ob["observations"][k]
            assert (fr[0, c] == random_shift(packed[:, 0], co)).all() and (fr[1, c] == random_shift(packed[:, 1], cn)).all(), (trial, k)
        assert (out.state[0].cpu().numpy() == ob["observations"]["state"][:, 0]).all()
        assert (out.action.cpu().numpy() == ob["actions"]).all() and (out.reward.cpu().numpy() == ob["rewards"]).all()
    cfg = O.Config(image_keys=keys, H=H, W=W, S=S, A=A)
    st, core = AH.make_pair(cfg, B)
    b = {"obs": {k: fr[0, c] for c, k in enumerate(keys)}, "next": {k: fr[1, c] for c, k in enumerate(keys)},
         "state": out.state[0].cpu().numpy(), "next_state": out.state[1].cpu().numpy(), "action": out.action.cpu().numpy(),
         "reward": out.reward.cpu().numpy(), "mask": out.mask.cpu().numpy()}
    noise = O.make_noise(cfg, B, seed=7)
    info, aux = O.update_critics(st, AH.batch_to_torch(b, torch.float64), O.noise_to_torch(noise, torch.float64))
    core.update_critics(out, AH.noise_to_device(cfg, noise))
    fig = _Figures("replay -> crop -> update_critics 84x96")
    _info(fig, core.read_info(), info, ("critic_loss", "predicted_qs", "target_qs"))
    _grads(fig, cfg, core, aux["grads"], "g_critic")
    fig.check()
    _compare_state(cfg, st, core)


def test_a_width_the_replay_rows_cannot_hold_is_refused_at_creation(gpu):
    """include/serl_mi355.h, serl_rb_create / serl_crop_packed: image rows are whole 16-byte vectors (W * 3 % 16 == 0).  84 columns
    are refused when the buffer is created and when a packed batch is cropped, with the limit in the message -- never in the
    middle of an update; the agents themselves take 84x84 through serl_batch (every other test of this file)."""
    from helpers import make_spaces
    from serl_amd._lib import SerlError
    from serl_amd.data.data_store import MemoryEfficientReplayBufferDataStore
    from serl_amd.utils.launcher import make_drq_agent
    osp, asp = make_spaces(("front",), 84, 84, 3, 1, 5, 3)
    with pytest.raises(SerlError, match=r"W\*C \(252\) must be a multiple of 16 bytes"):
        MemoryEfficientReplayBufferDataStore(osp, asp, 16, image_keys=("front",))
    # serl_crop_packed, reached by an agent that is handed a packed batch: refused before anything of the update has run
    B, S, A = 4, 5, 3
    obs0 = {"front": np.zeros((1, 84, 84, 3), np.uint8), "state": np.zeros((1, S), np.float32)}
    agent = make_drq_agent(5, obs0, np.zeros((A,), np.float32), image_keys=("front",), encoder_type="resnet-pretrained", batch_size=B)
    t = lambda a: torch.tensor(a, device="cuda")  # noqa: E731
    batch = {"observations": {"front": t(np.zeros((B, 2, 84, 84, 3), np.uint8)), "state": t(np.zeros((B, 1, S), np.float32))},
             "next_observations": {"state": t(np.zeros((B, 1, S), np.float32))}, "actions": t(np.zeros((B, A), np.float32)),
             "rewards": t(np.zeros(B, np.float32)), "masks": t(np.ones(B, np.float32))}
    before = agent.core.get("params", "critic/w1").copy()
    with pytest.raises(SerlError, match=r"W\*C \(252\) must be a multiple of 16 bytes"):
        agent.update_critics(batch)
    assert agent.core.step == 0 and np.array_equal(agent.core.get("params", "critic/w1"), before)
