"""Shared by tests/test_mlp_wide_{cpu,gpu}.py: MLP widths above 1024 (mlp_wide=True, serl_agent_opts.wide_widths; up to 4096), the
rows one workgroup of four waves owns (serl_amd/csrc/ln_wide.h).  The oracle, the storage cuts and the relu condition are
tests/mlp_ragged.py's; here are the case table, its oracle runs and a make_core with the switch."""
import torch

from oracle import drq_oracle as O
import agent_helpers as AH
import mlp_plain as MP
import mlp_ragged as MR
import policy_fixed as PF

installed = MR.installed
_D = dict(MR._D, ensemble=2, rows=6, utd=2, hw=0)
_D.pop("fixed_std")
CASES = {   # 17 chunks dealt 5/4/4/4; the maximum, K = 4096 into a narrow layer and back; rider, rank-1 backward and loss rider on a plain row
    "w1_1088_first_past_the_cap": dict(_D, rows=5, utd=5, critic_dims=(1088, 1088), policy_dims=(1088, 1088)),
    "w2_4096_64_E16_B65_swish": dict(_D, rows=65, ensemble=16, utd=5, critic_dims=(4096, 64), policy_dims=(64, 4096),
                                     critic_activation="swish", policy_activation="swish"),
    # (S = 200, A = 8: at S = 10 the 2048 relu units of a row lie too densely around 0 for any of 1500 seeds to keep the margin)
    "w3_plain_relu_critic_2048_one_row": dict(_D, S=200, A=8, rows=1, utd=0, critic_dims=(2048,), policy_dims=(1280,),
                                              critic_layer_norm=False, critic_activation="relu", seed=50),
    "w4_ragged_1025_4000": dict(_D, critic_dims=(1025, 4000), policy_dims=(300,)),      # stored 1088 and 4032 wide
    "w5_small_32x32_1536": dict(_D, kind="small", S=5, A=3, hw=32, critic_dims=(1536,), policy_dims=(1536,)),
}


def case_config(name):
    """-> (policy_fixed.FixedConfig, batch rows, the calls of the case, parameter seed)"""
    c = dict(CASES[name])
    rows, utd, seed, hw, kind = (c.pop(k) for k in ("rows", "utd", "seed", "hw", "kind"))
    img = dict(image_keys=("wrist",), H=hw, W=hw, encoder_type="small") if kind == "small" else dict(image_keys=(), discount=0.99)
    return PF.FixedConfig(hidden=c["critic_dims"][0], **img, **c), rows, ["critics", ("high_utd", 1)] + [("high_utd", utd)] * (utd > 1), seed


def make_core(cfg, B, seed=None, *, fuse=None, wide=True):
    """tests/mlp_ragged.py's make_core with wide_widths set (ragged_widths where a width is off the grid); seed: the parameters of
    the oracle runs loaded (inside installed())"""
    from serl_amd.agents.core import AgentCore
    with AH.chain_fuse(fuse):
        core = AgentCore(encoder_type=cfg.encoder_type, n_cam=cfg.n_cam, H=cfg.H, W=cfg.W, state_dim=cfg.S, act_dim=cfg.A, batch=B,
                         ensemble=cfg.ensemble, hidden=cfg.hidden, discount=cfg.discount, tau=cfg.tau, lr=cfg.lr, warmup_steps=cfg.warmup,
                         dropout=cfg.dropout, std_min=cfg.std_min, std_max=cfg.std_max, target_entropy=cfg.target_entropy,
                         critic_subsample_size=cfg.subsample, critic_activation=cfg.critic_activation, policy_activation=cfg.policy_activation,
                         critic_dims=cfg.critic_dims, policy_dims=cfg.policy_dims, critic_layer_norm=cfg.critic_layer_norm,
                         policy_layer_norm=cfg.policy_layer_norm, ragged=any(d % 64 for d in cfg.critic_dims + cfg.policy_dims), wide=wide)
    return core if seed is None else AH.load_leaves(core, cfg, *PF.init_params(cfg, seed))


_RUNS = {}


def oracle_run(name, call):
    """tests/mlp_ragged.py's oracle_run (fp64, same batch and noise seeds) on this table: computed once, unchanged by its readers"""
    if (name, call) not in _RUNS:
        cfg, B, _, seed = case_config(name)
        st, utd, d = O.TrainState(cfg, *PF.init_params(cfg, seed), torch.float64), 1 if call == "critics" else call[1], call != "critics"
        b, noise = AH.synth_batch(cfg, B, seed=3 + d), O.make_noise(cfg, B, seed=7 + d, utd_ratio=utd)
        with MP.relu_margin() as rec:
            tb, tn = AH.batch_to_torch(b, torch.float64), O.noise_to_torch(noise, torch.float64)
            info, aux = O.update_high_utd(st, tb, tn, utd) if d else O.update_critics(st, tb, tn)
        _RUNS[name, call] = dict(cfg=cfg, B=B, seed=seed, batch=b, noise=noise, state=st, info=info, aux=aux, relu=list(rec))
    return _RUNS[name, call]
