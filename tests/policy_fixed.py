"""Shared by tests/test_policy_fixed_cpu.py, tests/test_policy_fixed_gpu.py and tests/golden/make_golden_update_fixed.py: the
policy head with a fixed standard deviation (std_parameterization="fixed" with fixed_std, actor_critic_nets.py:189-192,212;
serl_agent_create_fixed_std, policy_fixed=True) -- the case table, the fp64 statement of the mode and the fixed_*.npz fixtures.

The fp64 statement.  oracle/drq_oracle.py states three std parameterisations.  "uniform" is the nearest: std = clip(exp(log_stds))
of one vector shared by all rows.  A fixed agent is that computation with the vector held at log(clip(fixed_std)) for ever, so the
oracle is run in "uniform" with actor/log_stds PINNED: set before the run, set back after every optimizer step (`pinned()` wraps
the oracle module's apply_gradients for the duration), and that leaf, its gradient and its moments left out of every comparison.
Adam is elementwise, so the pinned leaf's moments touch nothing else, and no other leaf's gradient depends on whether log_stds is a
parameter.  `pinned()` also looks at every policy evaluation: the oracle's std must equal clip(fixed_std) to 1e-15 in every row,
and tests/test_policy_fixed_cpu.py asserts that the oracle's OWN log_stds gradient is not zero -- a build that merely ran the uniform
agent would move that leaf.

A FixedConfig carries `fixed_std` (the float32 vector as Python floats) and reads std_parameterization "uniform" to the oracle; its
leaf table -- trainable_param_shapes / init_params below, on the oracle module under `installed()` -- is the uniform one WITHOUT
actor/log_stds, which is the fixed agent's arena.  pinned_config(cfg) is the Config the oracle's TrainState runs: the same, with
the leaf."""
import contextlib
import dataclasses
import os

import numpy as np
import torch

from oracle import drq_oracle as O
import agent_helpers as AH
import mlp_plain as MP
import mlp_shapes as MS

GOLDEN_DIR = MS.GOLDEN_DIR
LEAF = "actor/log_stds"      # the leaf the fp64 statement pins and every comparison leaves out
STD_TOL = 1e-15              # |oracle std - clip(fixed_std)| in every policy evaluation


@dataclasses.dataclass
class FixedConfig(MP.PlainConfig):
    fixed_std: tuple = None      # float32 values as Python floats, one per action column; None: no fixed agent

    def __post_init__(self):
        if self.fixed_std is not None:
            self.std_parameterization = "uniform"      # what the oracle runs, pinned
            self.fixed_std = tuple(float(np.float32(x)) for x in self.fixed_std)
            assert len(self.fixed_std) == self.A, (self.fixed_std, self.A)
        super().__post_init__()


def fixed_vector(fixed_std, A):
    """a scalar or a sequence -> the float32 vector of A entries the library holds"""
    return np.broadcast_to(np.asarray(fixed_std, np.float64).reshape(-1), (A,)).astype(np.float32)


def clip_fixed(cfg):
    """clip(fixed_std, std_min, std_max) as float64 [A]: the std of every row of every policy evaluation"""
    return np.clip(np.asarray(cfg.fixed_std, np.float64), cfg.std_min, cfg.std_max)


def pinned_config(cfg):
    """the "uniform" Config the oracle's TrainState runs for a fixed cfg: the same tree with actor/log_stds"""
    return dataclasses.replace(cfg, fixed_std=None, std_parameterization="uniform")


def trainable_param_shapes(cfg):
    """MP.trainable_param_shapes; a fixed Config has no std leaf at all; order == the arena's"""
    sh = MP.trainable_param_shapes(cfg)
    if getattr(cfg, "fixed_std", None) is not None:
        sh = {k: v for k, v in sh.items() if k != LEAF}
    return sh


def init_params(cfg, seed: int = 42, perturb: bool = True):
    """MP.init_params: the draws are those of the "exp" tree, so every shared leaf is the same; a fixed Config gets no std leaf"""
    trunk, theta = MP.init_params(cfg, seed, perturb)
    if getattr(cfg, "fixed_std", None) is not None:
        theta = {k: v for k, v in theta.items() if k != LEAF}
    return trunk, theta


_ORIG = {n: getattr(O, n) for n in ("trainable_param_shapes", "init_params", "policy_mlp", "critic_forward")}
GENERAL = {"trainable_param_shapes": trainable_param_shapes, "init_params": init_params, "policy_mlp": MP.policy_mlp,
           "critic_forward": MP.critic_forward}


@contextlib.contextmanager
def installed():
    """mlp_plain's general forward functions and the two leaf-table functions above on the imported oracle module, the originals
    back on every way out"""
    for n, f in GENERAL.items():
        setattr(O, n, f)
    try:
        yield
    finally:
        for n, f in _ORIG.items():
            setattr(O, n, f)


def pinned_theta(cfg, theta):
    """the fixed agent's leaves (oracle names) -> the pinned oracle's: actor/log_stds = log(clip(fixed_std)) in float64, in its
    arena position"""
    pin = np.log(clip_fixed(cfg))
    out = {}
    for k in trainable_param_shapes(pinned_config(cfg)):
        out[k] = pin if k == LEAF else theta[k]
    return out


def pinned_state(cfg, trunk, theta, dtype=torch.float64):
    """O.TrainState of pinned_config(cfg) from the fixed agent's leaves"""
    return O.TrainState(pinned_config(cfg), trunk, pinned_theta(cfg, theta), dtype)


@contextlib.contextmanager
def pinned(cfg):
    """For the duration the oracle module keeps actor/log_stds of every TrainState it steps at log(clip(fixed_std)) -- set back
    after every apply_gradients -- and every policy evaluation is looked at -> a record {"evaluations", "std_err" (worst
    |std - clip(fixed_std)|), "steps"}; an evaluation whose std is further than STD_TOL from clip(fixed_std) raises."""
    want = torch.tensor(clip_fixed(cfg), dtype=torch.float64)
    log_pin = torch.log(want)
    rec = {"evaluations": 0, "std_err": 0.0, "steps": 0}
    apply, head = O.apply_gradients, O.policy_head

    def apply_gradients(st, grads):
        apply(st, grads)
        st.params[LEAF] = log_pin.to(st.dtype).clone()
        rec["steps"] += 1

    def policy_head(th, c, enc):
        mean, std = head(th, c, enc)
        err = float((std.detach().to(torch.float64) - want).abs().max())
        rec["evaluations"] += 1
        rec["std_err"] = max(rec["std_err"], err)
        assert std.shape == mean.shape and err <= STD_TOL, (err, std[0], want)
        return mean, std
    O.apply_gradients, O.policy_head = apply_gradients, policy_head
    try:
        yield rec
    finally:
        O.apply_gradients, O.policy_head = apply, head


def unpinned(tree):
    """a {leaf: value} tree of the pinned oracle without the pinned leaf: what is compared"""
    return {k: v for k, v in tree.items() if k != LEAF}


def compared_state(st):
    """the pinned oracle's TrainState as tests/test_agent_gpu.py::_compare_state reads one (params, target), the pinned leaf dropped"""
    import types
    return types.SimpleNamespace(params=unpinned(st.params), target=unpinned(st.target), step=st.step)


# ---- the case table: the smallest shapes at which each route of the fixed mode can go wrong ----------------------------------------
# id -> dict(kind, S, A, rows, ensemble, utd (> 1, or 0: none), squash, backup_entropy, fixed_std (scalar or vector), std_min,
#            std_max, critic_dims, policy_dims, critic_layer_norm)
# kind: "state", "frozen1" (one camera 64x64 on the frozen ResNet-10 trunk), "small" (one camera 64x64, SmallEncoder).
# (a) two columns clipped: 0.01 < std_min = 0.05 and 5.0 > std_max = 2; 72 rows = two 64-row head tiles, the second ragged.
# (b) the plain Gaussian with backup_entropy: alpha * logp is in the critic target while logp has no parameter gradient.
# (c) one action column, one row.  (d) A = 64: policy_stats_kernel's one lane per column at its limit; 65 rows leave one row in
# a last 256-thread pass of the row loops and one in a second head tile; the vector runs from below std_min to above std_max.
# (e), (f) the two pixel agents.  (g) the head's K follows the policy's last width (128) beside a plain one-layer critic.
_D = dict(S=10, ensemble=10, squash=True, backup_entropy=False, std_min=1e-5, std_max=5.0, critic_dims=(256, 256), policy_dims=(256, 256),
          critic_layer_norm=True)
CASES = {
    "a_state_two_columns_clipped": dict(_D, kind="state", A=5, rows=72, utd=2, fixed_std=(0.01, 0.3, 1.0, 5.0, 0.7), std_min=0.05, std_max=2.0),
    "b_state_gauss_backup_entropy": dict(_D, kind="state", A=5, rows=72, utd=2, fixed_std=0.1, squash=False, backup_entropy=True),
    "c_state_one_column_one_row": dict(_D, kind="state", A=1, rows=1, utd=0, fixed_std=0.5, ensemble=2),
    "d_state_64_columns_65_rows": dict(_D, kind="state", A=64, rows=65, utd=5, fixed_std=tuple(np.geomspace(0.02, 4.0, 64)), std_min=0.05,
                                       std_max=2.0, ensemble=2),
    "e_frozen_one_camera": dict(_D, kind="frozen1", S=5, A=3, rows=6, utd=2, fixed_std=(0.2, 0.05, 1.5)),
    "f_small_one_camera_gauss": dict(_D, kind="small", S=5, A=3, rows=6, utd=2, fixed_std=0.3, squash=False),
    "g_state_shapes_plain_critic": dict(_D, kind="state", A=4, rows=8, utd=2, fixed_std=0.1, critic_dims=(320,), policy_dims=(64, 128),
                                        critic_layer_norm=False),
}
IDS = list(CASES)
PARAM_SEED = 42


def config(kind, S, A, fixed_std, *, ensemble=10, squash=True, backup_entropy=False, std_min=1e-5, std_max=5.0, critic_dims=(256, 256),
           policy_dims=(256, 256), critic_layer_norm=True, **kw):
    common = dict(S=S, A=A, ensemble=ensemble, tanh_squash=squash, backup_entropy=backup_entropy, std_min=std_min, std_max=std_max,
                  critic_dims=tuple(critic_dims), policy_dims=tuple(policy_dims), critic_layer_norm=critic_layer_norm,
                  hidden=critic_dims[0], fixed_std=tuple(fixed_vector(fixed_std, A).tolist()), **kw)
    if kind == "state":
        return FixedConfig(image_keys=(), discount=0.99, **common)
    if kind == "frozen1":
        return FixedConfig(image_keys=("wrist",), H=64, W=64, **common)
    assert kind == "small", kind
    return FixedConfig(image_keys=("wrist",), H=64, W=64, encoder_type="small", **common)


def case_config(name):
    """-> (FixedConfig, batch rows, utd > 1 or 0)"""
    c = dict(CASES[name])
    rows, utd = c.pop("rows"), c.pop("utd")
    return config(c.pop("kind"), c.pop("S"), c.pop("A"), c.pop("fixed_std"), **c), rows, utd


def make_pair(cfg, B, dtype=torch.float64, seed=PARAM_SEED, agent_seed=0, trunk_mode=None, fuse=None):
    """-> (pinned oracle TrainState, fixed AgentCore) holding identical shared leaves; inside installed()"""
    trunk, theta = init_params(cfg, seed)
    core = AH.make_core(cfg, B, fuse=fuse, trunk_mode=trunk_mode, agent_seed=agent_seed)
    return pinned_state(cfg, trunk, theta, dtype), AH.load_leaves(core, cfg, trunk, theta)


# ---- the oracle runs of a case, computed once per (case, call) and shared by the tests that need them ------------------------------
_RUNS = {}


def calls_of(name):
    """the update calls the parity tests make on a case"""
    utd = CASES[name]["utd"]
    return ["critics", ("high_utd", 1)] + ([("high_utd", utd)] if utd > 1 else [])


def oracle_run(name, call):
    """call: "critics", or ("high_utd", utd) -> {"cfg", "B", "batch", "noise", "state" (the pinned TrainState after the call), "info",
    "aux", "pin" (pinned()'s record)}; inside installed().  Unchanged by its readers.  Batch and noise seeds: tests/mlp_plain.py's."""
    key = (name, call)
    if key not in _RUNS:
        cfg, B, _ = case_config(name)
        trunk, theta = init_params(cfg, PARAM_SEED)
        st = pinned_state(cfg, trunk, theta)
        pc = st.cfg
        with pinned(cfg) as rec:
            if call == "critics":
                b, noise = AH.synth_batch(pc, B, seed=3), O.make_noise(pc, B, seed=7)
                info, aux = O.update_critics(st, AH.batch_to_torch(b, torch.float64), O.noise_to_torch(noise, torch.float64))
            else:
                utd = call[1]
                b, noise = AH.synth_batch(pc, B, seed=4), O.make_noise(pc, B, seed=8, utd_ratio=utd)
                info, aux = O.update_high_utd(st, AH.batch_to_torch(b, torch.float64), O.noise_to_torch(noise, torch.float64), utd)
        _RUNS[key] = dict(cfg=cfg, B=B, batch=b, noise=noise, state=st, info=info, aux=aux, pin=rec)
    return _RUNS[key]


# ---- the reference's call of the create functions ----------------------------------------------------------------------------------
def policy_kwargs(cfg, fixed_std=None):
    """the launcher's policy_kwargs (utils/launcher.py:55-60) in the fixed mode of a FixedConfig; fixed_std: another form of the
    same vector (a scalar)"""
    return {"tanh_squash_distribution": cfg.tanh_squash, "std_parameterization": "fixed",
            "fixed_std": list(cfg.fixed_std) if fixed_std is None else fixed_std, "std_min": cfg.std_min, "std_max": cfg.std_max}


def reference_agent(cfg, B, **kw):
    """golden_replay.reference_agent at a FixedConfig: the reference's kwargs through mlp_shapes, mlp_plain and policy_fixed"""
    import golden_replay as GR
    args = dict(policy_kwargs=policy_kwargs(cfg), mlp_shapes=True, mlp_plain=True, policy_fixed=True, **MP.network_kwargs(cfg))
    args.update(kw)
    return GR.reference_agent(cfg, B, **args)


def sac_agent(fixed_std, seed=0, B=8, S=10, A=5, squash=True, std_min=1e-5, std_max=5.0, **kw):
    """make_sac_agent's call of SACAgent.create_states (launcher.py:50-76) with a fixed-std policy_kwargs and policy_fixed=True"""
    import mlp_widths as MW
    pk = {"tanh_squash_distribution": squash, "std_parameterization": "fixed", "fixed_std": fixed_std, "std_min": std_min, "std_max": std_max}
    args = dict(policy_kwargs=pk, policy_fixed=True)
    args.update(kw)
    return MW.sac_agent(256, seed=seed, B=B, S=S, A=A, **args)


# ---- tests/golden/fixed_*.npz (tests/golden/make_golden_update_fixed.py) ------------------------------------------------------------
# name -> (case, schedule).  The Configs are the cases' with the optimizers of the launcher's state-only factory (warm-up 2000,
# the temperature's none), as golden_replay.STATE has them.
GOLDEN = {
    "update_sac_state": ("a_state_two_columns_clipped", [("high_utd", 2), ("update", ("actor", "critic", "temperature")), ("high_utd", 1)]),
    "update_sac_state_gauss": ("b_state_gauss_backup_entropy", [("high_utd", 2), ("update", ("actor", "critic", "temperature")), ("high_utd", 1)]),
    "update_drq": ("e_frozen_one_camera", [("critics",), ("high_utd", 2)]),
}
GAUSS_VECTOR = (0.1, 0.25, 0.1, 0.4, 0.1)      # fixed_update_sac_state_gauss.npz: case (b) with a length-A vector
N_SAMPLE = 1024


def golden_config(name):
    """-> (FixedConfig, rows, schedule) of fixture `name`"""
    import golden_replay as GR
    case, sched = GOLDEN[name]
    c = dict(CASES[case])
    rows = c.pop("rows")
    c.pop("utd")
    kind, S, A, fixed = c.pop("kind"), c.pop("S"), c.pop("A"), c.pop("fixed_std")
    if name == "update_sac_state_gauss":
        fixed = GAUSS_VECTOR
    if kind == "state":
        assert (S, A) == (GR.STATE["S"], GR.STATE["A"])
        c.update(warmup=2000, temp_warmup=GR.STATE["temp_warmup"])
    cfg = config(kind, S, A, fixed, **c)
    if kind != "state":
        cfg = dataclasses.replace(cfg, image_keys=("image",))      # the key the launcher's drq fixtures use
    return cfg, rows, sched


def golden_path(name):
    return os.path.join(GOLDEN_DIR, f"fixed_{name}.npz")


def load_golden(name):
    """-> (oracle.golden_update.unpack of fixed_<name>.npz with g["cfg"] the FixedConfig of golden_config(name), meta, npz)"""
    from oracle import golden_update as G
    z = np.load(golden_path(name))
    g = G.unpack(z)
    cfg, rows, sched = golden_config(name)
    assert g["B"] == rows and [s["kind"] for s in g["steps"]] == [s[0] for s in sched]
    g["cfg"] = cfg
    return g, g["meta"], z


def initial_leaves(cfg):
    """-> (trunk, theta) a fixed_*.npz run started from, oracle names: O.init_params of the launcher's tree at golden_replay.PARAM_SEED
    without the std leaves"""
    import golden_replay as GR
    return init_params(cfg, GR.PARAM_SEED)
