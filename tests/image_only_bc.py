"""Shared by tests/test_image_only_bc_cpu.py and tests/test_image_only_bc_gpu.py: the behaviour-cloning agent without the proprio
branch (BCAgent.create(use_proprio=False), the reference's own default, bc.py:126; serl_bc_opts.no_proprio).

The fp64 statement is tests/bc_oracle.py, unmodified: `installed()` puts tests/image_only.py's `encode` on the oracle module (the
image codes alone: `state` is never touched) and takes the four enc/proprio leaves out of bc_oracle.TRAIN for the duration, so that
State, update and the step checks of tests/test_learner_regimes_gpu.py walk the eight leaves that train: the two MLP layers and the
two heads.  actor/w1 has 256 * n_cam rows (image_only.ImageOnlyConfig.enc_dim)."""
import contextlib

import numpy as np
import torch

from oracle import drq_oracle as O
import bc_oracle as BO
import image_only as IO

TRAIN = tuple(k for k in BO.TRAIN if not k.startswith("enc/proprio/"))
_TRAIN_ORIG = BO.TRAIN


@contextlib.contextmanager
def installed():
    with IO.installed():
        BO.TRAIN = TRAIN
        try:
            yield
        finally:
            BO.TRAIN = _TRAIN_ORIG


# (id, cameras, H, W, rows, A): one row and one action column; two cameras off the tile sizes, across the 64-row GEMM tile
CASES = [("one_cam_B1_A1", ("wrist",), 32, 32, 1, 1), ("two_cams_33x47_B65_A5", ("wrist", "front"), 33, 47, 65, 5)]
IDS = [c[0] for c in CASES]
S = 5


def case_config(case, use_proprio=False):
    _, keys, H, W, B, A = case
    return IO.ImageOnlyConfig(image_keys=keys, H=H, W=W, S=S, A=A, use_proprio=use_proprio), B


def theta_of(cfg, seed=42):
    """(trunk, the BC leaves) of an image-only Config; inside installed()"""
    trunk, theta = IO.init_params(cfg, seed)
    return trunk, BO.bc_theta(theta)


def inputs(cfg, B, seed):
    """-> {"frames", "state", "action", "masks"} of one update, actions near enough to the policy for a finite loss"""
    rng = np.random.default_rng(seed)
    return {"frames": {k: rng.integers(0, 256, (B, cfg.H, cfg.W, 3), dtype=np.uint8) for k in cfg.image_keys},
            "state": rng.standard_normal((B, cfg.S)).astype(np.float32),
            "action": rng.uniform(-1, 1, (B, cfg.A)).astype(np.float32),
            "masks": {k: (rng.random((B, cfg.sle_dim)) < 1.0 - cfg.dropout).astype(np.uint8) for k in cfg.image_keys}}


_RUNS = {}


def run(case, dtype=torch.float64, steps=2):
    """`steps` updates from theta_of on inputs(seed 70 + i) -> [{"info", "grads", "aux", "inp"} per step], "state" after the last;
    memoised, read-only; inside installed()"""
    key = (case[0], str(dtype), steps)
    if key not in _RUNS:
        cfg, B = case_config(case)
        trunk, theta = theta_of(cfg)
        st = BO.State(cfg, trunk, theta, dtype)
        out = []
        for i in range(steps):
            inp = inputs(cfg, B, 70 + i)
            info, grads, aux = BO.update(st, BO.features(trunk, cfg, inp["frames"], dtype), inp["state"], inp["action"], inp["masks"])
            out.append({"info": info, "grads": {k: g.double().numpy() for k, g in grads.items()}, "inp": inp,
                        "aux": {k: v.double().numpy() for k, v in aux.items()}})
        _RUNS[key] = {"steps": out, "state": st, "trunk": trunk, "theta": theta, "cfg": cfg, "B": B}
    return _RUNS[key]


def bc_agent(cfg, B, trunk, theta, use_proprio=False):
    from serl_amd import jaxrng as J
    from serl_amd.agents.bc import BCAgent
    agent = BCAgent(cfg.image_keys, cfg.H, cfg.W, cfg.S, cfg.A, seed_key=J.prngkey(0), max_batch=B, use_proprio=use_proprio)
    agent.load_flat(trunk)
    agent.load_flat(theta)
    return agent


def create(image_keys=("wrist",), H=32, W=32, A=3, B=4, seed=0, **kw):
    """BCAgent.create as the launcher calls it (utils/launcher.py:26-47), with the reference's own use_proprio default unless said"""
    from serl_amd.agents.bc import BCAgent
    obs = {k: np.zeros((H, W, 3), np.uint8) for k in image_keys}
    obs["state"] = np.zeros((S,), np.float32)
    args = dict(encoder_type="resnet-pretrained", image_keys=tuple(image_keys), batch_size=B,
                network_kwargs={"activations": "tanh", "use_layer_norm": False, "hidden_dims": [256, 256]},
                policy_kwargs={"tanh_squash_distribution": False, "std_parameterization": "exp", "std_min": 1e-5, "std_max": 5})
    args.update(kw)
    return BCAgent.create(seed, obs, np.zeros((A,), np.float32), **args)


# ---- tests/golden/imgonly_bc_64.npz (tests/golden/make_golden_bc_image_only.py): the reference's own BCAgent.create(use_proprio=False) ----
GOLDEN = "imgonly_bc_64"


def golden():
    """-> (npz, meta, ImageOnlyConfig) of imgonly_bc_64.npz"""
    import json
    import os
    from oracle import golden_update as G
    d = np.load(os.path.join(IO.GOLDEN_DIR, f"{GOLDEN}.npz"))
    meta = json.loads(str(d["meta"]))
    return d, meta, IO.ImageOnlyConfig(**G.cfg_from_dict(meta["cfg"]).__dict__, use_proprio=bool(meta["image_only"]["use_proprio"]))


def golden_masks(d, cfg, i, B):
    return {k: np.unpackbits(d[f"s{i}_mask_{k}"])[:B * 4096].reshape(B, 4096) for k in cfg.image_keys}
