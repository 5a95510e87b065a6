"""ctypes declarations of the handle half of the C ABI (include/serl_mi355.h): the agent, BC and reward-classifier
handles.  _lib.lib() applies SIGNATURES / RESTYPES once, when it loads the library."""
import ctypes as C

from ._lib import P, SerlBatch, f32, i32, i64, vp
from .utils.init import MAX_MLP_LAYERS


class SerlAgentCfg(C.Structure):
    _fields_ = [
        ("device", C.c_int), ("n_cam", C.c_int), ("H", C.c_int), ("W", C.c_int),
        ("state_dim", C.c_int), ("act_dim", C.c_int), ("batch", C.c_int), ("ensemble", C.c_int),
        ("hidden", C.c_int), ("bottleneck", C.c_int), ("sle_features", C.c_int),
        ("proprio_dim", C.c_int), ("warmup_steps", C.c_int), ("temp_warmup_steps", C.c_int),
        ("discount", C.c_float), ("tau", C.c_float), ("lr", C.c_float), ("dropout", C.c_float),
        ("std_min", C.c_float), ("std_max", C.c_float), ("target_entropy", C.c_float),
        ("seed", C.c_uint64),
        # per-optimizer options of make_optimizer (common/optimizers.py:6-56), index = TX_INDEX[name]
        ("tx_lr", C.c_float * 3), ("tx_warmup", C.c_int * 3), ("tx_cosine_steps", C.c_int * 3),
        ("tx_weight_decay_on", C.c_int * 3), ("tx_weight_decay", C.c_float * 3), ("tx_clip_norm", C.c_float * 3),
        ("encoder_type", C.c_int),   # 0 = resnet-pretrained (frozen trunk), 1 = small (trainable SmallEncoder)
        ("critic_subsample_size", C.c_int),   # 0 = 2, -1 = None (all members), else 1..16
        ("backup_entropy", C.c_int),
        ("tx_lr_set", C.c_int * 3),   # != 0: tx_lr[t] given explicitly (0.0 is a valid optax learning rate)
        ("num_stack", C.c_int),   # T, frames per observation (0 = 1); state_dim is then the flattened width T * S
    ]


class SerlMlpOpts(C.Structure):      # serl_mlp_opts: one network's MLP; all zero = two LayerNorm+tanh layers of cfg.hidden, no Dropout
    _fields_ = [("act", C.c_int), ("n_layers", C.c_int), ("dims", C.c_int * MAX_MLP_LAYERS), ("no_layer_norm", C.c_int),
                ("dropout", C.c_double)]


class SerlAgentOpts(C.Structure):    # serl_agent_opts (utils.init.NetSpec.to_c fills it); all zero = serl_agent_create(cfg)
    _fields_ = [("std_param", C.c_int), ("no_tanh", C.c_int), ("critic", SerlMlpOpts), ("policy", SerlMlpOpts),
                ("fixed_std", P(C.c_float)), ("ragged_widths", C.c_int), ("no_proprio", C.c_int)]


TX_INDEX = {"actor": 0, "critic": 1, "temperature": 2}   # SERL_TX_*
NET_BITS = {"critic": 1, "actor": 2, "temperature": 4}   # SERL_NET_*
APPLY_CRITIC, APPLY_ACTOR_TEMP = NET_BITS["critic"], NET_BITS["actor"] | NET_BITS["temperature"]   # SERL_APPLY_*


class SerlBcCfg(C.Structure):
    _fields_ = [
        ("device", C.c_int), ("n_cam", C.c_int), ("H", C.c_int), ("W", C.c_int), ("state_dim", C.c_int),
        ("act_dim", C.c_int), ("max_batch", C.c_int),
        ("lr", C.c_float), ("dropout", C.c_float), ("std_min", C.c_float), ("std_max", C.c_float),
    ]


class SerlBcOpts(C.Structure):       # serl_bc_opts; all zero = serl_bc_create(cfg)
    _fields_ = [("no_proprio", C.c_int)]


class SerlClassifierCfg(C.Structure):
    _fields_ = [("device", C.c_int), ("n_cam", C.c_int), ("H", C.c_int), ("W", C.c_int), ("max_batch", C.c_int)]


class SerlNoise(C.Structure):
    _fields_ = [
        ("eps_next", C.c_void_p), ("mask_next", C.c_void_p), ("redq_idx", C.c_void_p),
        ("eps_pi", C.c_void_p), ("mask_obs_pi", C.c_void_p),
        ("eps_temp", C.c_void_p), ("mask_next_temp", C.c_void_p),
        # jax.random keys (host uint32 words) instead of tensors: serl_mi355.h "Round 5"
        ("key_eps_next", C.c_void_p), ("key_mask_next", C.c_void_p), ("key_eps_pi", C.c_void_p), ("key_mask_obs_pi", C.c_void_p),
        ("key_eps_temp", C.c_void_p), ("key_mask_next_temp", C.c_void_p),
    ]


MLP_SITES = ("pi_next", "q_target", "q_online", "pi", "q_actor", "pi_temp")   # SERL_SITE_*, in code order
MLP_CRITIC_LOSS_SITES = MLP_SITES[:3]      # one draw per critic update of a call
MLP_SITE_NETWORK = {"pi_next": "policy", "q_target": "critic", "q_online": "critic", "pi": "policy", "q_actor": "critic", "pi_temp": "policy"}


class SerlMlpNoise(C.Structure):      # serl_mlp_noise
    _fields_ = [("mask", C.c_void_p * len(MLP_SITES)), ("key", C.c_void_p * len(MLP_SITES)), ("mask_rows", C.c_int32)]


class SerlInfo(C.Structure):
    _fields_ = [(n, C.c_float) for n in (
        "critic_loss", "predicted_qs", "target_qs", "actor_loss", "temperature", "entropy",
        "temperature_loss", "actor_lr", "critic_lr", "temperature_lr")]


class SerlSnapshotMeta(C.Structure):   # serl_snapshot_meta
    _fields_ = [("step", C.c_int64), ("trunk_gen", C.c_int64), ("bytes", C.c_int64), ("nonfinite", C.c_int64 * 3),
                ("sections", C.c_int), ("slots", C.c_int)]


SNAP_BITS = {"params": 1, "target_params": 2, "opt_states": 4}   # SERL_SNAP_*, by the TrainState field each bit fills

# function -> argtypes (int status unless RESTYPES says otherwise)
SIGNATURES = {
    "serl_agent_create_opts": [P(SerlAgentCfg), P(SerlAgentOpts), P(vp)],   # what AgentCore calls; the older entry points follow
    "serl_agent_create": [P(SerlAgentCfg), P(vp)],
    "serl_agent_create_policy": [P(SerlAgentCfg), i32, i32, P(vp)],   # std_param (SERL_STD_*), no_tanh
    "serl_agent_create_mlp": [P(SerlAgentCfg), i32, i32, i32, i32, P(vp)],   # ... critic_act, policy_act (SERL_ACT_*)
    "serl_agent_create_dropout": [P(SerlAgentCfg), i32, i32, i32, i32, C.c_double, C.c_double, P(vp)],   # ... critic_dropout, policy_dropout
    # ... critic_dims, n_critic, policy_dims, n_policy (hidden_dims of each network; no Dropout)
    "serl_agent_create_shapes": [P(SerlAgentCfg), i32, i32, i32, i32, P(i32), i32, P(i32), i32, P(vp)],
    "serl_agent_create_layer_norm": [P(SerlAgentCfg), i32, i32, i32, i32, P(i32), i32, P(i32), i32, i32, i32, P(vp)],   # ... critic_layer_norm, policy_layer_norm
    "serl_agent_mlp_layer_norm": [vp, i32],   # network (0 critic, 1 policy) -> 1 / 0
    # serl_agent_create_layer_norm's arguments, then fixed_std: act_dim floats with std_param SERL_STD_FIXED (3), NULL otherwise
    "serl_agent_create_fixed_std": [P(SerlAgentCfg), i32, i32, i32, i32, P(i32), i32, P(i32), i32, i32, i32, P(C.c_float), P(vp)],
    "serl_agent_fixed_std": [vp, P(C.c_float)],   # out: act_dim floats, the vector as passed
    "serl_agent_mlp_dims": [vp, i32, P(i32)],   # network (0 critic, 1 policy), dims[SERL_MAX_MLP_LAYERS] -> layer count
    "serl_agent_set_mlp_noise": [vp, P(SerlMlpNoise)],
    "serl_agent_destroy": [vp],
    "serl_agent_live_trunk": [vp],
    "serl_agent_use_proprio": [vp],   # 1 / 0 (serl_agent_opts.no_proprio) / -1
    "serl_agent_num_leaves": [vp],
    "serl_agent_leaf_info": [vp, i32, C.c_char_p, i32, P(i64)],
    "serl_agent_leaf_layout": [vp, C.c_char_p, P(i64)],   # out[5] = n, rows, cols, rows_p, ld (serl_mi355.h)
    "serl_agent_set": [vp, C.c_char_p, C.c_char_p, vp, i64],
    "serl_agent_get": [vp, C.c_char_p, C.c_char_p, vp, i64],
    "serl_agent_set_step": [vp, i64],
    "serl_agent_set_trunk_mode": [vp, i32],
    "serl_agent_set_chain_budget": [vp, i32],
    "serl_agent_get_step": [vp],
    "serl_agent_update_critics": [vp, P(SerlBatch), P(SerlNoise), vp],
    "serl_agent_update_high_utd": [vp, P(SerlBatch), i32, P(SerlNoise), vp],
    "serl_agent_read_info": [vp, P(SerlInfo), vp],
    "serl_agent_encode": [vp, P(SerlBatch), vp],
    "serl_agent_encode_slot": [vp, P(SerlBatch), i32, vp],
    "serl_agent_encode_slot_range": [vp, P(SerlBatch), i32, i32, i32, vp],
    "serl_agent_select_slot": [vp, i32],
    "serl_agent_slot_features": [vp, i32, P(vp), P(i64)],
    "serl_agent_bind_slot": [vp, P(SerlBatch), i32],
    "serl_agent_critic_grads": [vp, i32, i32, i32, P(SerlNoise), i32, vp],
    "serl_agent_critic_grads_bucketed": [vp, i32, i32, i32, P(SerlNoise), i32, vp, vp],
    "serl_agent_grad_bucket": [vp, i32, P(vp), P(i64)],
    "serl_agent_actor_grads": [vp, i32, P(SerlNoise), vp],
    "serl_agent_apply": [vp, i32, f32, vp],
    "serl_agent_update": [vp, P(SerlBatch), i32, P(SerlNoise), vp],
    "serl_agent_begin_update": [vp, vp],
    "serl_agent_set_shard": [vp, i64, i64],
    "serl_agent_grad_view": [vp, i32, P(vp), P(i64)],
    "serl_agent_sample_actions": [vp, vp, vp, i32, vp, vp, vp],
    # read-only evaluation: forward_critic / forward_target_critic, forward_policy, loss_fns without the step
    "serl_agent_eval_q": [vp, vp, vp, vp, i32, i32, vp, vp],
    "serl_agent_eval_policy": [vp, vp, vp, vp, i32, vp, vp, vp, vp, vp],
    "serl_agent_eval_losses": [vp, P(SerlBatch), P(SerlNoise), P(SerlInfo), vp],
    "serl_agent_trunk_forward": [vp, vp, i32, vp, vp],
    "serl_agent_debug_get": [vp, C.c_char_p, vp, i64],
    "serl_agent_trunk_plan": [vp, C.c_char_p, i32],
    "serl_agent_debug_set": [vp, C.c_char_p, vp, i64],
    "serl_debug_chain_launches": [],
    # parameter snapshots (csrc/snapshot.hip, serl_amd/agents/snapshot.py)
    "serl_snapshot_create": [vp, i32, i32, P(vp)],
    "serl_snapshot_take": [vp, vp, P(i32)],
    "serl_snapshot_ready": [vp, i32],
    "serl_snapshot_wait": [vp, i32],
    "serl_snapshot_info": [vp, i32, P(SerlSnapshotMeta)],
    "serl_snapshot_leaf": [vp, i32, C.c_char_p, C.c_char_p, P(P(f32)), P(i64)],
    "serl_snapshot_release": [vp, i32],
    "serl_snapshot_destroy": [vp],
    # behaviour cloning (csrc/bc.hip, serl_amd/agents/bc.py)
    "serl_bc_create": [P(SerlBcCfg), P(vp)],
    "serl_bc_create_opts": [P(SerlBcCfg), P(SerlBcOpts), P(vp)],
    "serl_bc_use_proprio": [vp],
    "serl_bc_destroy": [vp],
    "serl_bc_num_leaves": [vp],
    "serl_bc_leaf_info": [vp, i32, C.c_char_p, i32, P(i64), P(i32)],
    "serl_bc_set": [vp, C.c_char_p, C.c_char_p, vp, i64],
    "serl_bc_get": [vp, C.c_char_p, C.c_char_p, vp, i64],
    "serl_bc_set_step": [vp, i64],
    "serl_bc_get_step": [vp],
    "serl_bc_update": [vp, P(SerlBatch), vp, vp, vp],
    "serl_bc_read_info": [vp, vp, vp],
    "serl_bc_sample_actions": [vp, vp, vp, i32, vp, vp, f32, i32, vp, vp],
    "serl_bc_debug_metrics": [vp, P(SerlBatch), vp, vp, vp, vp],
    # reward classifier (csrc/classifier.hip, serl_amd/networks/reward_classifier.py)
    "serl_classifier_create": [P(SerlClassifierCfg), P(vp)],
    "serl_classifier_destroy": [vp],
    "serl_classifier_num_leaves": [vp],
    "serl_classifier_leaf_info": [vp, i32, C.c_char_p, i32, P(i64)],
    "serl_classifier_set": [vp, C.c_char_p, vp, i64],
    "serl_classifier_get": [vp, C.c_char_p, vp, i64],
    "serl_classifier_logits": [vp, vp, i32, vp, vp],
    "serl_classifier_logits_from_features": [vp, vp, i64, P(i32), i32, vp, vp],
    # reward labelling inside the DrQ update (vice.py:546,594)
    "serl_agent_set_reward_classifier": [vp, vp, P(i32), P(i32)],
    "serl_agent_label_rewards": [vp, vp],
    "serl_agent_reward_label_rows": [vp],
    "serl_agent_read_reward_labels": [vp, vp, vp, P(f32), vp],
    "serl_classifier_train_init": [vp, i32, f32, f32, f32, f32],
    "serl_classifier_train_step": [vp, vp, i32, vp, vp, vp, vp],
    "serl_classifier_train_forward": [vp, vp, i32, vp, vp, vp, vp],
    "serl_classifier_read_train_info": [vp, vp, vp],
    "serl_classifier_train_set_step": [vp, i64],
    "serl_classifier_train_get_step": [vp, P(i64)],
    "serl_classifier_train_set": [vp, C.c_char_p, C.c_char_p, vp, i64],
    "serl_classifier_train_get": [vp, C.c_char_p, C.c_char_p, vp, i64],
}
RESTYPES = {"serl_agent_get_step": i64, "serl_bc_get_step": i64, "serl_debug_chain_launches": i64}
