"""Shared by tests/test_mlp_widths_cpu.py and tests/test_mlp_widths_gpu.py: the table of MLP widths (serl_agent_cfg.hidden,
hidden_dims=[h, h]) the parity tests run, the reference's create calls at a width, and the reader of
tests/golden/widths_init_*.npz (tests/golden/make_golden_update_widths.py; widths_update_*.npz: golden_replay.load_variant)."""
import ast
import os

import numpy as np

from oracle import drq_oracle as O
from oracle import golden_update as G

GOLDEN_DIR = os.path.join(os.path.dirname(__file__), "golden")
UPDATE_GOLDEN = ("sac_state_w128", "drq_w320")
INIT_GOLDEN = "sac_state_w128"

# (id, hidden, kind, batch rows, ensemble, the UTD > 1 the row runs; 0 = none: the fp64 oracle of 16 members at 1024 takes seconds
# per pass, and 1024 has its UTD > 1 in the frozen-trunk row).  One wave owns a LayerNorm row, so a lane holds hidden / 64
# columns: 1 = the minimum; 3 = no 16-byte access, below 256; 5 = above 256, odd; 8; 16 = the maximum and the largest scratch.
# Rows are no multiple of the four rows a LayerNorm workgroup takes (7 = one partial workgroup and a 64-row GEMM tile with 57
# empty rows, 65 = one tile and one row); ensembles 3 and 16 (16 = the most a state-only agent takes: 16 members x 65 rows x 1024
# columns is the largest slab image); A = 3.  kind: "state" (no encoder), "frozen" (one camera 32x32, ResNet-10 trunk),
# "small" (one camera 33x47, SmallEncoder).
CASES = [
    ("w64_state_B7_E3", 64, "state", 7, 3, 7),
    ("w192_frozen_B65_E16", 192, "frozen", 65, 16, 5),
    ("w320_small_B7_E3", 320, "small", 7, 3, 7),
    ("w512_state_B65_E3", 512, "state", 65, 3, 13),
    ("w1024_state_B65_E16", 1024, "state", 65, 16, 0),
    ("w1024_frozen_B7_E3", 1024, "frozen", 7, 3, 7),
]
IDS = [c[0] for c in CASES]


def config(hidden, kind, ensemble=10):
    if kind == "state":
        return O.Config(image_keys=(), S=10, A=3, discount=0.99, hidden=hidden, ensemble=ensemble)
    if kind == "frozen":
        return O.Config(image_keys=("wrist",), H=32, W=32, S=5, A=3, hidden=hidden, ensemble=ensemble)
    return O.Config(image_keys=("wrist",), H=33, W=47, S=5, A=3, hidden=hidden, ensemble=ensemble, encoder_type="small")


def case_config(case):
    """-> (oracle Config, batch rows, utd > 1)"""
    _, hidden, kind, B, ensemble, utd = case
    return config(hidden, kind, ensemble), B, utd


def init_golden():
    """tests/golden/widths_init_sac_state_w128.npz in the form of init_golden_helpers.load: (npz, cfg, {leaf: (name, record)},
    {leaf: shape})"""
    import init_golden_helpers as IG
    z = np.load(os.path.join(GOLDEN_DIR, f"widths_init_{INIT_GOLDEN}.npz"))
    assert int(z["widths_n_sample"]) == IG.N_SAMPLE
    cfg = G.cfg_from_dict(ast.literal_eval(bytes(z["init_cfg"]).decode()))
    leaves = {}
    for k in z.files:
        if k.startswith("init/"):
            name, part = k[5:].rsplit("/", 1)
            leaves.setdefault(name, {})[part] = z[k]
    shapes = {k[11:]: tuple(int(s) for s in z[k]) for k in z.files if k.startswith("init_shape/")}
    return z, cfg, {k: (k, v) for k, v in leaves.items()}, shapes


def mlp_kwargs(h, **kw):
    """the launcher's critic_network_kwargs / policy_network_kwargs (utils/launcher.py:50-116) at width h"""
    return {"activations": "tanh", "use_layer_norm": True, "hidden_dims": [h, h], **kw}


POLICY_KWARGS = {"tanh_squash_distribution": True, "std_parameterization": "exp", "std_min": 1e-5, "std_max": 5}


def sac_agent(h, seed=0, B=8, S=10, A=4, **kw):
    """make_sac_agent's call of SACAgent.create_states (launcher.py:50-76) with hidden_dims=[h, h]"""
    from serl_amd.agents.sac import SACAgent
    args = dict(policy_kwargs=dict(POLICY_KWARGS), critic_network_kwargs=mlp_kwargs(h), policy_network_kwargs=mlp_kwargs(h),
                temperature_init=1e-2, discount=0.99, backup_entropy=False, critic_ensemble_size=10, critic_subsample_size=2,
                batch_size=B)
    args.update(kw)
    return SACAgent.create_states(seed, np.zeros((S,), np.float32), np.zeros((A,), np.float32), **args)


def drq_agent(h, keys, H, W, S, A, seed=0, B=8, encoder_type="resnet-pretrained", **kw):
    """make_drq_agent's call of DrQAgent.create_drq (launcher.py:79-116) with hidden_dims=[h, h]"""
    from serl_amd.agents.drq import DrQAgent
    obs = {k: np.zeros((1, H, W, 3), np.uint8) for k in keys}
    obs["state"] = np.zeros((1, S), np.float32)
    args = dict(encoder_type=encoder_type, use_proprio=True, image_keys=keys, policy_kwargs=dict(POLICY_KWARGS),
                critic_network_kwargs=mlp_kwargs(h), policy_network_kwargs=mlp_kwargs(h), temperature_init=1e-2, discount=0.96,
                backup_entropy=False, critic_ensemble_size=10, critic_subsample_size=2, batch_size=B)
    args.update(kw)
    return DrQAgent.create_drq(seed, obs, np.zeros((A,), np.float32), **args)
