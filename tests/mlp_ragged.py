"""Shared by tests/test_mlp_ragged_cpu.py and tests/test_mlp_ragged_gpu.py: critic and policy MLP widths off the 64 grid
(serl_agent_opts.ragged_widths, mlp_ragged=True; any width in [1, 1024]).

The oracle is the shape-general fp64 one of tests/mlp_shapes.py with the LayerNorm flags of tests/mlp_plain.py and the pinned
fixed-std statement of tests/policy_fixed.py (whose `installed()` puts all of it on the oracle module): it takes any width as it
stands.  A layer of true width d is stored 64 ceil(d / 64) wide on the device; nothing here knows that except `storage`, which
cuts a leaf's own elements out of the two gradient taps -- the one place where a test reads storage instead of a leaf.

The case table.  Rows are 6, 65 or 72.  The widths meet each LayerNorm row layout with a ragged tail: 50 and 3 are stored 64 wide
(the one-column-per-lane kernel), 200 is stored 256 wide (the blocked kernel, pads in the last lanes), 65, 100, 127, 300, 400 and
1000 take the strided kernel at 2, 2, 2, 5, 7 and 16 columns per lane.  The seeds of the relu cases are chosen on the CPU so that
every relu pre-activation of the fp64 oracle keeps tests/mlp_plain.py's RELU_MARGIN from 0 (tests/test_mlp_ragged_cpu.py asserts it)."""
import contextlib

import numpy as np
import torch

from oracle import drq_oracle as O
import agent_helpers as AH
import mlp_plain as MP
import policy_fixed as PF

installed = PF.installed

# id -> dict(kind, S, A, rows, ensemble, utd (> 1, or 0), critic_dims, policy_dims, critic_layer_norm, policy_layer_norm,
#            critic_activation, policy_activation, fixed_std (None: the launcher's exp head), seed)
_D = dict(kind="state", S=10, A=4, ensemble=10, utd=2, critic_layer_norm=True, policy_layer_norm=True, critic_activation="tanh",
          policy_activation="tanh", fixed_std=None, seed=42)
CASES = {
    "r1_state_400_300": dict(_D, A=5, rows=72, ensemble=2, critic_dims=(400, 300), policy_dims=(400, 300)),
    "r1_state_400_300_td3": dict(_D, A=5, rows=72, ensemble=2, critic_dims=(400, 300), policy_dims=(400, 300), fixed_std=0.1),
    "r2_state_65_127": dict(_D, rows=6, critic_dims=(65, 127), policy_dims=(127, 65)),
    "r3_state_1000_50_E16_B65": dict(_D, rows=65, ensemble=16, utd=5, critic_dims=(1000, 50), policy_dims=(50, 1000)),
    "r4_state_one_layer_critic_200": dict(_D, rows=6, ensemble=3, critic_dims=(200,), policy_dims=(3, 200, 100, 64)),
    "r5_state_plain_relu_critic_beside_ln_swish_policy": dict(_D, rows=6, ensemble=2, critic_dims=(100, 100), policy_dims=(200,),
                                                              critic_layer_norm=False, critic_activation="relu", policy_activation="swish",
                                                              seed=71),
    "r5_state_ln_tanh_critic_beside_plain_relu_policy": dict(_D, rows=6, ensemble=2, critic_dims=(100, 100), policy_dims=(200,),
                                                             policy_layer_norm=False, policy_activation="relu", seed=45),
    "r5_state_plain_swish_critic_beside_ln_relu_policy": dict(_D, rows=6, ensemble=2, critic_dims=(200,), policy_dims=(100, 100),
                                                              critic_layer_norm=False, critic_activation="swish", policy_activation="relu",
                                                              seed=42),
    "r6_frozen_100_200__300": dict(_D, kind="frozen1", S=5, A=3, rows=6, critic_dims=(100, 200), policy_dims=(300,)),
    "r6_small_100_200__300": dict(_D, kind="small", S=5, A=3, rows=6, ensemble=2, critic_dims=(100, 200), policy_dims=(300,)),
}
IDS = list(CASES)


def case_config(name):
    """-> (policy_fixed.FixedConfig, batch rows, utd > 1 or 0, parameter seed)"""
    c = dict(CASES[name])
    rows, utd, seed, fixed = c.pop("rows"), c.pop("utd"), c.pop("seed"), c.pop("fixed_std")
    kind, S, A = c.pop("kind"), c.pop("S"), c.pop("A")
    if fixed is not None:
        return PF.config(kind, S, A, fixed, **c), rows, utd, seed
    common = dict(S=S, A=A, hidden=c["critic_dims"][0], **c)
    if kind == "state":
        return PF.FixedConfig(image_keys=(), discount=0.99, **common), rows, utd, seed
    if kind == "frozen1":
        return PF.FixedConfig(image_keys=("wrist",), H=64, W=64, **common), rows, utd, seed
    return PF.FixedConfig(image_keys=("wrist",), H=64, W=64, encoder_type="small", **common), rows, utd, seed


def make_core(cfg, B, *, fuse=None, trunk_mode=None, agent_seed=0, ragged=True):
    """agent_helpers.make_core with serl_agent_opts.ragged_widths set"""
    from serl_amd.agents.core import AgentCore
    fixed = getattr(cfg, "fixed_std", None)
    with AH.chain_fuse(fuse):
        core = AgentCore(encoder_type=cfg.encoder_type, n_cam=cfg.n_cam, H=cfg.H, W=cfg.W, state_dim=cfg.S, act_dim=cfg.A, batch=B,
                         ensemble=cfg.ensemble, hidden=cfg.hidden, discount=cfg.discount, tau=cfg.tau, lr=cfg.lr,
                         warmup_steps=cfg.warmup, dropout=cfg.dropout, std_min=cfg.std_min, std_max=cfg.std_max,
                         target_entropy=cfg.target_entropy, seed=agent_seed,
                         temp_warmup_steps=-1 if cfg.temp_warmup is None else cfg.temp_warmup,
                         critic_subsample_size=cfg.subsample, backup_entropy=cfg.backup_entropy, optimizers=cfg.opt,
                         std_parameterization=cfg.std_parameterization if fixed is None else "fixed",
                         fixed_std=None if fixed is None else np.asarray(fixed, np.float32), tanh_squash_distribution=cfg.tanh_squash,
                         critic_activation=cfg.critic_activation, policy_activation=cfg.policy_activation,
                         critic_dims=getattr(cfg, "critic_dims", None), policy_dims=getattr(cfg, "policy_dims", None),
                         critic_layer_norm=getattr(cfg, "critic_layer_norm", True), policy_layer_norm=getattr(cfg, "policy_layer_norm", True),
                         ragged=ragged)
    if trunk_mode is not None:
        core.set_trunk_mode(trunk_mode)
    return core


def oracle_state(cfg, trunk, theta, dtype=torch.float64):
    """the TrainState the oracle runs: the pinned one of a fixed Config (policy_fixed.py), the Config's own otherwise"""
    return PF.pinned_state(cfg, trunk, theta, dtype) if cfg.fixed_std is not None else O.TrainState(cfg, trunk, theta, dtype)


def make_pair(cfg, B, dtype=torch.float64, seed=42, fuse=None, ragged=True):
    """-> (oracle TrainState, ragged AgentCore) holding identical leaves; inside installed()"""
    trunk, theta = PF.init_params(cfg, seed)
    return oracle_state(cfg, trunk, theta, dtype), AH.load_leaves(make_core(cfg, B, fuse=fuse, ragged=ragged), cfg, trunk, theta)


_RUNS = {}


def calls_of(name):
    utd = CASES[name]["utd"]
    return ["critics", ("high_utd", 1)] + ([("high_utd", utd)] if utd > 1 else [])


def oracle_run(name, call, dtype=torch.float64):
    """call: "critics" or ("high_utd", utd) -> {"cfg", "B", "seed", "batch", "noise", "state" (the TrainState after the call, the
    pinned leaf of a fixed case dropped: policy_fixed.compared_state), "info", "aux", "relu" (min |relu pre-activation| per
    evaluated layer)}; computed once, inside installed(), unchanged by its readers.  Batch and noise seeds: tests/mlp_plain.py's."""
    key = (name, call, dtype)
    if key not in _RUNS:
        cfg, B, _, seed = case_config(name)
        trunk, theta = PF.init_params(cfg, seed)
        st = oracle_state(cfg, trunk, theta, dtype)
        pc = st.cfg
        with (PF.pinned(cfg) if cfg.fixed_std is not None else contextlib.nullcontext()), MP.relu_margin() as rec:
            if call == "critics":
                b, noise = AH.synth_batch(pc, B, seed=3), O.make_noise(pc, B, seed=7)
                info, aux = O.update_critics(st, AH.batch_to_torch(b, dtype), O.noise_to_torch(noise, dtype))
            else:
                utd = call[1]
                b, noise = AH.synth_batch(pc, B, seed=4), O.make_noise(pc, B, seed=8, utd_ratio=utd)
                info, aux = O.update_high_utd(st, AH.batch_to_torch(b, dtype), O.noise_to_torch(noise, dtype), utd)
        if cfg.fixed_std is not None:
            st = PF.compared_state(st)
            aux = {k: (PF.unpinned(v) if k in ("grads", "g_actor") else v) for k, v in aux.items()}
        _RUNS[key] = dict(cfg=cfg, B=B, seed=seed, batch=b, noise=noise, state=st, info=info, aux=aux, relu=list(rec))
    return _RUNS[key]


def check_relu_margin(name):
    """tests/mlp_plain.py's condition: every relu pre-activation of every fp64 oracle run of the case is at least RELU_MARGIN from 0"""
    c = CASES[name]
    worst = float("inf")
    for call in calls_of(name):
        run = oracle_run(name, call)
        assert bool(run["relu"]) == ("relu" in (c["critic_activation"], c["policy_activation"])), (name, call)
        for m in run["relu"]:
            assert m >= MP.RELU_MARGIN, f"{name} {call}: a relu pre-activation lies {m:.3g} from 0 (< {MP.RELU_MARGIN:g})"
            worst = min(worst, m)
    return worst


# ---- storage: where a leaf lies in the padded gradient taps -----------------------------------------------------------------------
def storage(core):
    """{leaf: (offset, (n, rows, cols, rows_p, ld))} of the trainable leaves in the order of the arena, offsets in floats of
    STORAGE: what serl_agent_grad_view and the "g_critic" / "g_actor" taps are indexed by (serl_agent_leaf_layout)"""
    out, off = {}, 0
    for leaf in core.leaves:
        if leaf.startswith("trunk/"):
            continue
        lay = core.leaf_layout(leaf)
        out[leaf] = (off, lay)
        off += lay[0] * lay[3] * lay[4]
    return out


def tap_ranges(core):
    """-> {"g_critic": (lo, hi), "g_actor": (lo, hi)}: the storage range each gradient tap covers (csrc/agent.hip's Pc, Pa0, Pa1)"""
    st = storage(core)
    end = lambda k: st[k][0] + st[k][1][0] * st[k][1][3] * st[k][1][4]      # noqa: E731
    names = list(st)
    last_actor = [k for k in names if k.startswith("actor/")][-1]
    return {"g_critic": (0, end("enc/proprio/ln/bias" if "enc/proprio/ln/bias" in st else "critic/head/bias")),
            "g_actor": (st["enc/proprio/dense/kernel" if "enc/proprio/dense/kernel" in st else "actor/w1"][0], end(last_actor))}


def cut(flat, lo, entry):
    """the leaf's own elements, dense, out of a tap that starts at storage offset lo"""
    off, (n, rows, cols, rows_p, ld) = entry
    return flat[off - lo:off - lo + n * rows_p * ld].reshape(n, rows_p, ld)[:, :rows, :cols].reshape(-1)


def pads(flat, lo, entry):
    """the padding of the leaf's storage in the same tap"""
    off, (n, rows, cols, rows_p, ld) = entry
    box = flat[off - lo:off - lo + n * rows_p * ld].reshape(n, rows_p, ld)
    return np.concatenate([box[:, :rows, cols:].reshape(-1), box[:, rows:, :].reshape(-1)])


def grads(fig, cfg, core, want, tap):
    """tests/test_mlp_widths_gpu.py::_grads through `storage`: every gradient leaf of `want` against the tap, AH.rel_err at the
    figure's tolerance; and the padding of every leaf inside the tap is exactly zero"""
    lo, hi = tap_ranges(core)[tap]
    g = core.debug(tap, hi - lo)
    st = storage(core)
    for k, gv in want.items():
        entry = st[AH.product_name(k, cfg.image_keys)]
        fig.add(f"{tap} {k}", AH.rel_err(cut(g, lo, entry), gv.numpy().reshape(-1)))
        assert not pads(g, lo, entry).any(), (tap, k)


SECTIONS = ("params", "target_params", "opt/critic/mu", "opt/critic/nu", "opt/actor/mu", "opt/actor/nu", "opt/temperature/mu",
            "opt/temperature/nu")


def all_bits(core):
    return {(sec, leaf): core.get(sec, leaf).copy() for leaf in core.leaves for sec in SECTIONS}


# ---- the reference's call of the create functions -----------------------------------------------------------------------------------
def network_kwargs(cfg):
    return MP.network_kwargs(cfg)


def sac_agent(critic_dims, policy_dims, seed=0, B=8, S=10, A=4, **kw):
    """make_sac_agent's call of SACAgent.create_states (launcher.py:50-76) with the two hidden_dims, mlp_shapes and mlp_ragged on"""
    import mlp_shapes as MS
    return MS.sac_agent(critic_dims, policy_dims, seed=seed, B=B, S=S, A=A, mlp_ragged=True, **kw)


# ---- tests/golden/ragged_*.npz (tests/golden/make_golden_update_ragged.py): the format of tests/golden/shapes_*.npz ---------------------
import mlp_shapes as MS  # noqa: E402

PARAM_SEED, BATCH_SEED = 42, 100
UPDATE_GOLDEN = ("sac_state", "drq")


def golden_update_cases():
    """name -> (mlp_shapes.ShapeConfig, batch rows, schedule, sampled elements per large leaf)"""
    import golden_replay as GR
    return {
        "sac_state": (MS.ShapeConfig(critic_dims=(400, 300), policy_dims=(400, 300), warmup=2000, **GR.STATE), 72, list(GR.STATE_SCHED), 512),
        "drq": (MS.ShapeConfig(image_keys=("image",), H=64, W=64, S=5, A=3, critic_dims=(100, 200), policy_dims=(300,)), 6,
                [("critics",), ("high_utd", 2)], 1024),
    }


def golden_init_case():
    import golden_replay as GR
    return MS.ShapeConfig(critic_dims=(100, 50), policy_dims=(65, 127, 3), warmup=2000, **GR.STATE), 8, [("high_utd", 1)]


def load_golden(name):
    """-> oracle.golden_update.unpack of ragged_update_<name>.npz, g["cfg"] a ShapeConfig"""
    import os
    from oracle import golden_update as G
    g = G.unpack(np.load(os.path.join(MS.GOLDEN_DIR, f"ragged_update_{name}.npz")))
    g["cfg"] = MS._with_dims(g["cfg"], g["meta"])
    return g


def init_golden():
    """ragged_init_sac_state.npz in the form of init_golden_helpers.load: (npz, cfg, {leaf: (name, record)}, {leaf: shape})"""
    import ast
    import json
    import os
    import init_golden_helpers as IG
    from oracle import golden_update as G
    z = np.load(os.path.join(MS.GOLDEN_DIR, "ragged_init_sac_state.npz"))
    assert int(z["shapes_n_sample"]) == IG.N_SAMPLE
    cfg = MS._with_dims(G.cfg_from_dict(ast.literal_eval(bytes(z["init_cfg"]).decode())), json.loads(str(z["meta"])))
    leaves = {}
    for k in z.files:
        if k.startswith("init/"):
            name, part = k[5:].rsplit("/", 1)
            leaves.setdefault(name, {})[part] = z[k]
    shapes = {k[11:]: tuple(int(s) for s in z[k]) for k in z.files if k.startswith("init_shape/")}
    return z, cfg, {k: (k, v) for k, v in leaves.items()}, shapes


def reference_agent(cfg, B, **kw):
    """golden_replay.reference_agent with the Config's two lists through mlp_shapes=True and mlp_ragged=True"""
    import golden_replay as GR
    return GR.reference_agent(cfg, B, critic_network_kwargs=MS.mlp_kwargs(cfg.critic_dims), policy_network_kwargs=MS.mlp_kwargs(cfg.policy_dims),
                              mlp_shapes=True, mlp_ragged=True, **kw)
