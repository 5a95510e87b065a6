/* serl_mi355.h -- C ABI of libserl_mi355.so, the MI355X (gfx950) learner hot path for SERL.
 *
 * The reference (rail-berkeley/serl) is pure Python/JAX and has no FFI seam; the seam is the
 * Python object API used by the learner loop (examples/async_drq_sim/async_drq_sim.py:183-311).
 * Each entry point below replaces the reference method(s) cited next to it; INTEGRATION.md shows
 * the ctypes stub a maintainer would add on the reference side.  All paths are relative to
 * serl_launcher/serl_launcher/ in the reference tree.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error; serl_last_error() gives the message
 *     (thread-local).  No exceptions, no Python or torch types cross this boundary.
 *   - "dev" pointers are device (HBM) addresses owned by the caller (e.g. torch tensors'
 *     data_ptr()); "host" pointers are ordinary host memory.  `stream` is a hipStream_t passed
 *     as void* (0 = null stream).  Kernels are enqueued asynchronously on it.
 *   - handles own their device memory (hipMalloc) and are freed by the matching *_destroy.
 */
#ifndef SERL_MI355_H
#define SERL_MI355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SERL_OK 0
#define SERL_ERR_INVALID (-1)
#define SERL_ERR_HIP (-2)
#define SERL_ERR_STATE (-3)
#define SERL_ERR_UNSUPPORTED (-4)

#define SERL_MAX_CAMS 4
#define SERL_MAX_BUFFERS 2

const char* serl_last_error(void);
int serl_version(void);
/* number of visible HIP devices (0 if none); does not fail without a GPU */
int serl_device_count(void);

/* HIP-event timing of the hot kernels (off by default).  serl_profile_enable(k): k = 0 off, k >= 1 times every
 * k-th launch of each instrumented tag (an event pair costs a few microseconds on the stream, which matters
 * once the step itself is below a millisecond).  serl_profile_read returns, per tag, the summed duration and
 * the number of TIMED launches since the last reset:
 * names is char[max_entries][64]. Used by bench.py for the live roofline numbers. */
int serl_profile_enable(int on);
int serl_profile_reset(void);
int serl_profile_read(int max_entries, char* names, double* total_ms, int64_t* counts, int* n_out);

/* ------------------------------------------------------------------------------------------
 * Replay buffer  (data/memory_efficient_replay_buffer.py, data/replay_buffer.py, data/dataset.py)
 * Frames live in HBM: one u8[H*W*C] frame per slot per camera (the *next* frame of the
 * transition; observation frame of slot i is slot i-1), plus one f32 record per slot.
 * ------------------------------------------------------------------------------------------ */
typedef struct serl_rb serl_rb;

/* MemoryEfficientReplayBuffer.__init__ (memory_efficient_replay_buffer.py:13-51) +
 * ReplayBuffer.__init__ (replay_buffer.py:41-66). num_stack = T (frames per observation).
 * LIMIT: image rows are whole 16-byte vectors, W * C % 16 == 0 (with C = 3: W a multiple of 16; H is free) -- any other
 * width is refused here with SERL_ERR_INVALID ("W*C (...) must be a multiple of 16 bytes"). */
int serl_rb_create(int device, int64_t capacity, int n_cam, int H, int W, int C, int num_stack,
                   int state_dim, int act_dim, serl_rb** out);
int serl_rb_destroy(serl_rb* rb);

/* Dataset.seed (dataset.py:72-74): the caller builds numpy's PCG64(SeedSequence(seed)) and hands
 * over its raw state (bit_generator.state), so SeedSequence hashing stays in numpy. */
int serl_rb_seed(serl_rb* rb, uint64_t state_hi, uint64_t state_lo, uint64_t inc_hi,
                 uint64_t inc_lo, int has_uint32, uint32_t uinteger);
/* read back the generator state (tests: must equal numpy's after the same draws) */
int serl_rb_rng_state(serl_rb* rb, uint64_t out_state_inc[4], int* has_uint32, uint32_t* uinteger);

/* MemoryEfficientReplayBuffer.insert (memory_efficient_replay_buffer.py:53-89), thread-safe like
 * MemoryEfficientReplayBufferDataStore.insert (data_store.py:104-106).
 * obs_frames[c] / next_frames[c]: host u8[T][H][W][C] for camera c; state/next_state: host
 * f32[T*S]; action: host f32[A].  A NULL array, table or table entry is SERL_ERR_INVALID (the entries are checked since the
 * argument checks are shared with serl_rb_insert_batch). */
int serl_rb_insert(serl_rb* rb, const uint8_t* const* obs_frames,
                   const uint8_t* const* next_frames, const float* state,
                   const float* next_state, const float* action, float reward, float mask,
                   int done);

/* n calls of serl_rb_insert, in order, with byte-identical results (frames, records, valid mask, size, insert_index,
 * insert_count, first; the sampler's generator is not touched) -- what an actor's message or a file of demonstrations brings.
 * obs_frames / next_frames: [n * n_cam] host pointers, entry i*n_cam + c -> u8[T][H][W][C] (NULL tables for a store without
 * cameras); state, next_state f32[n][T*S]; action f32[n][A]; reward, mask f32[n]; done u8[n].
 * Every argument is checked before anything is inserted: n < 0, a NULL array or a NULL table entry is SERL_ERR_INVALID and leaves
 * the store untouched; n == 0 succeeds and does nothing.  The slot writes are staged in slots of 2 MB and go to HBM with ONE
 * host-to-device copy and ONE kernel launch per staging slot, whatever the number of cameras (a payload that wraps the ring or
 * overwrites its own slots takes a few more launches).  The store's mutex is released between transitions only: another thread's
 * index draw, gather or snapshot export sees each transition wholly or not at all.  Where it releases the mutex the call stands
 * back, for at most 100 us, while an index draw or a gather of another thread waits for it: inserts yield priority to readers.
 * "Untouched" covers the argument checks only: a HIP error in the middle of a payload (SERL_ERR_HIP) leaves the bookkeeping and
 * serl_rb_insert_stats advanced for transitions whose data may not have reached HBM, exactly as a HIP error inside
 * serl_rb_insert does -- such a store is to be discarded. */
int serl_rb_insert_batch(serl_rb* rb, int n, const uint8_t* const* obs_frames, const uint8_t* const* next_frames,
                         const float* state, const float* next_state, const float* action,
                         const float* reward, const float* mask, const uint8_t* done);
/* out = { transitions inserted, serl_rb_insert_batch calls, H2D copies enqueued by inserts, kernel launches enqueued by inserts } */
int serl_rb_insert_stats(serl_rb* rb, int64_t out[4]);

int64_t serl_rb_len(serl_rb* rb);          /* ReplayBuffer.__len__ (replay_buffer.py:68-69) */
int64_t serl_rb_insert_index(serl_rb* rb); /* latest_data_id (data_store.py:138-140) */
int serl_rb_valid_mask(serl_rb* rb, uint8_t* host_out /* [capacity] */);
/* Slot writes ever made: every ReplayBuffer.insert of the reference (replay_buffer.py:71-75), i.e. each time the write head
 * advances -- a transition's own slot, an episode's first-frame slots and the wrap re-inserts all count.  insert_index ==
 * count % capacity, and unlike insert_index it never wraps, so "the slots written since count c" is the ring range
 * [c % capacity, count % capacity) as long as count - c < capacity. */
int64_t serl_rb_insert_count(serl_rb* rb);

/* ---- Snapshot of a store (run resume).  Everything in a store that is state rather than workspace: the geometry, the ring
 * bookkeeping, the sampler's PCG64, the valid mask, and the frames and records of the slots. */
typedef struct serl_rb_meta {
  int64_t capacity;
  int32_t n_cam, H, W, C, T, S, A, rec_len;  /* rec_len = 2*T*S + A + 3 floats per record */
  int64_t size, insert_index, insert_count;
  int32_t first;                             /* the next insert opens an episode (writes first-frame slots) */
  int32_t rng_seeded;
  uint64_t rng_state_inc[4];                 /* as serl_rb_rng_state */
  int32_t rng_has_uint32;
  uint32_t rng_uinteger;
} serl_rb_meta;
/* One consistent reading of all of the above (under the store's mutex: never between the slot writes of one insert). */
int serl_rb_export_meta(serl_rb* rb, serl_rb_meta* out);
/* Copies the n_slots slots slot_begin, slot_begin + 1, ... (mod capacity: the range may run over the end of the ring) to host
 * memory, in that order: host_frames[c] u8[n_slots][H*W*C] per camera (NULL for a store without cameras), host_records
 * f32[n_slots][rec_len], and -- when host_valid is not NULL -- the WHOLE valid mask u8[capacity]: an insert changes the mask of
 * slots other than the one it writes (look-ahead invalidation, first-frame slots, the wrap re-insert), so a saver may keep
 * frames incrementally but must rewrite the mask whole.  0 <= slot_begin < capacity, 0 <= n_slots <= capacity.
 * Ordering: the call first waits for the copies of the last insert, then reads device memory in chunks through pinned staging
 * on the store's copy stream.  While it runs, inserts into the store (and other exports / imports) WAIT -- every insert is
 * either wholly in the result or not at all; index draws and gathers on any stream proceed (they only read). */
int serl_rb_export_slots(serl_rb* rb, int64_t slot_begin, int64_t n_slots, uint8_t* const* host_frames,
                         float* host_records, uint8_t* host_valid);
/* The inverse.  serl_rb_import_meta sets the bookkeeping and the generator; the geometry in `meta` (capacity, n_cam, H, W, C, T,
 * S, A, rec_len) must be the store's own, and size / insert_index / insert_count consistent with it, else SERL_ERR_INVALID and
 * the store is untouched.  serl_rb_import_slots writes a slot range (same layout and limits as the export; host_valid, when not
 * NULL, replaces the whole mask) host -> HBM in chunks through pinned staging, after the gathers in flight that may read those
 * slots, and refreshes the host mirror of the records that the wrap re-insert reads.  It holds the store's mutex throughout and
 * returns when the copies have completed: nothing else touches the store meanwhile. */
int serl_rb_import_meta(serl_rb* rb, const serl_rb_meta* meta);
int serl_rb_import_slots(serl_rb* rb, int64_t slot_begin, int64_t n_slots, const uint8_t* const* host_frames,
                         const float* host_records, const uint8_t* host_valid);

/* index draw + rejection loop (memory_efficient_replay_buffer.py:111-122): bit-exact with
 * numpy Generator(PCG64).integers.  host_idx_out: int64[batch]. */
int serl_rb_sample_indices(serl_rb* rb, int batch, int64_t* host_idx_out);

/* gather of sample(pack_obs_and_next_obs=True) (memory_efficient_replay_buffer.py:126-164,
 * dataset.py:40-51).  dev outputs:  frames_out[c] u8[batch][T+1][H][W][C];
 * state_out/next_state_out f32[batch][T*S]; action_out f32[batch][A]; reward_out, mask_out
 * f32[batch]; done_out u8[batch].  host_idx: int64[batch] slot indices, IN/OUT: an index whose slot an insert has invalidated
 * since it was drawn is re-drawn (from the buffer's generator) and written back, so the array always describes the batch
 * that was gathered.  Gathers may be issued from several streams; an insert that overwrites a slot waits for all of them. */
int serl_rb_gather_packed(serl_rb* rb, int64_t* host_idx, int batch,
                          uint8_t* const* dev_frames_out, float* dev_state_out,
                          float* dev_next_state_out, float* dev_action_out,
                          float* dev_reward_out, float* dev_mask_out, uint8_t* dev_done_out,
                          void* stream);

/* Device batch consumed by the agent: the result of sample -> [concat_batches] -> _unpack ->
 * random-shift crop.  All pointers are device addresses owned by the caller.
 *   frames : u8 [2 (0=obs,1=next)][n_cam][batch][T][H][W][C]   (frame-planar: frame t of a stack is a whole H*W*C image)
 *   state  : f32[2][batch][state_dim], state_dim = T * S (the T proprio vectors of a stack, oldest first)
 * T = num_stack (0 means 1, so a zero-initialised struct describes the single-frame batch it always did).  Observation frame
 * t is frame t of the packed T+1 window and next-observation frame t is frame t+1 (utils/train_utils.py:53-64).
 */
typedef struct serl_batch {
  int batch, n_cam, H, W, C, state_dim, act_dim;
  uint8_t* frames;
  float* state;
  float* action;
  float* reward;
  float* mask;
  uint8_t* done;
  int num_stack;           /* T: frames per observation; 0 = 1 */
} serl_batch;

/* Fused sample-gather + concat_batches + _unpack + DrQ random shift (K2+K3+K4 of SURVEY.md):
 * memory_efficient_replay_buffer.py:126-164 + utils/train_utils.py:16-31,44-66 +
 * vision/data_augmentations.py:7-36 + agents/continuous/drq.py:244-253 (same offsets for every
 * camera).  Samples [0,counts[0]) come from rbs[0], the next counts[1] from rbs[1] (RLPD 50/50).
 * host_crop_obs / host_crop_next: int32[batch*T][2] = (dy,dx) in [0,8], entry b*T + t for frame t of sample b (every frame of
 * a stack has its own offset: batched_random_crop with num_batch_dims=2 splits its key B*T ways); NULL = no shift (4,4).
 * host_idx[b]: IN/OUT like serl_rb_gather_packed's (stale indices are re-drawn in place).
 * Stores with num_stack T > 1 need out->num_stack == T and out->state_dim == T * S (SERL_ERR_INVALID otherwise). */
int serl_rb_gather_crop(serl_rb* const* rbs, int n_rb, int64_t* const* host_idx,
                        const int* counts, const int32_t* host_crop_obs,
                        const int32_t* host_crop_next, const serl_batch* out, void* stream);

/* _unpack + random shift on an already-gathered packed batch (train_utils.py:44-66,
 * data_augmentations.py:7-36): dev_packed[c] u8[batch][2][H][W][C] -> out->frames.  Same LIMIT as serl_rb_create:
 * W * C % 16 == 0, refused otherwise (the agents themselves take any H, W >= 32 through serl_batch). */
int serl_crop_packed(int device, const uint8_t* const* dev_packed, int n_cam, int batch, int H,
                     int W, int C, const int32_t* host_crop_obs, const int32_t* host_crop_next,
                     uint8_t* dev_frames_out, void* stream);
/* The same for frame stacks: dev_packed[c] u8[batch][T+1][H][W][C] -> dev_frames_out u8[2][n_cam][batch][T][H][W][C], observation
 * frame t = packed frame t, next frame t = packed frame t+1; crop tables int32[batch*T][2] (entry b*T + t), NULL = no shift.
 * 1 <= num_stack <= 4.  serl_crop_packed is this function with num_stack == 1. */
int serl_crop_packed_stacked(int device, const uint8_t* const* dev_packed, int n_cam, int batch, int num_stack, int H,
                             int W, int C, const int32_t* host_crop_obs, const int32_t* host_crop_next,
                             uint8_t* dev_frames_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * DrQ / SAC agent  (agents/continuous/drq.py, agents/continuous/sac.py, common/common.py)
 * One handle = JaxRLTrainState (params, target_params, 3 Adam states, step) + all activations.
 * ------------------------------------------------------------------------------------------ */
typedef struct serl_agent serl_agent;

/* hyper-parameters of make_drq_agent / DrQAgent.create_drq (utils/launcher.py:79-116,
 * agents/continuous/drq.py:24-242) with encoder_type == "resnet-pretrained". */
typedef struct serl_agent_cfg {
  int device;
  int n_cam, H, W;         /* image_keys order is the caller's; C == 3.  n_cam == 0: state-only SAC
                            * (SACAgent.create_states, sac.py:486-542): no encoder, observations are the flat
                            * state vectors, one Dense(1) Q head per ensemble member; H, W ignored */
  int state_dim, act_dim;
  int batch;               /* max samples per update call on THIS rank */
  int ensemble;            /* critic_ensemble_size (10) */
  int hidden;              /* width of the critic's and the policy's two MLP layers, hidden_dims = [hidden, hidden]: a multiple of
                              64 in [64, 1024] (256 in the launcher's configurations); anything else is SERL_ERR_INVALID */
  int bottleneck;          /* encoder bottleneck_dim: 256 (create_drq fixes it), anything else is SERL_ERR_INVALID */
  int sle_features;        /* num_spatial_blocks (8) */
  int proprio_dim;         /* proprio_latent_dim (64) */
  int warmup_steps;        /* optimizers.py:23-30: actor and critic optimizers (0 for DrQ, 2000 for make_sac_agent) */
  int temp_warmup_steps;   /* temperature optimizer's own warm-up; < 0: same as warmup_steps (sac.py:333-343: none) */
  float discount, tau, lr;
  float dropout;           /* 0.1, resnet_v1.py:351 */
  float std_min, std_max;  /* 1e-5, 5 */
  float target_entropy;    /* -act_dim/2, drq.py:88-89 */
  uint64_t seed;           /* device noise stream (production mode) */
  /* Per-optimizer options of make_optimizer (common/optimizers.py:6-56), indexed by SERL_TX_*.  All zero (the
   * default, what every example uses) = adam + the warm-up -> constant schedule above.
   *   tx_lr            > 0: learning rate of this optimizer (else `lr`); with tx_lr_set[t] != 0 the value is taken as
   *                    given, 0 included (optax accepts learning_rate=0.0, e.g. to freeze the temperature)
   *   tx_warmup       >= 0: warm-up steps of this optimizer, given as steps + 1 (0 = use warmup_steps / temp_warmup_steps)
   *   tx_cosine_steps  > 0: warmup_cosine_decay_schedule(0, lr, warmup, decay_steps = this, end 0) (optimizers.py:14-21)
   *   tx_weight_decay_on != 0: optax.adamw with tx_weight_decay (optimizers.py:39-42); it decays the WHOLE tree, as the
   *                    reference's tx.update(grads, state, params) does -- on an agent with the pretrained ResNet-10 that
   *                    tree holds the "frozen" trunk too: see LIVE TRUNK at serl_agent_create_opts
   *   tx_clip_norm     > 0: optax.clip_by_global_norm on this optimizer's gradient tree (optimizers.py:36-37) */
  float tx_lr[3];
  int tx_warmup[3];
  int tx_cosine_steps[3];
  int tx_weight_decay_on[3];
  float tx_weight_decay[3];
  float tx_clip_norm[3];
  /* encoder_type of DrQAgent.create_drq (drq.py:137-186): SERL_ENCODER_RESNET_PRETRAINED (0, the frozen ResNet-10 of
   * every example) or SERL_ENCODER_SMALL: the trainable SmallEncoder (vision/small_encoders.py:9-55, features
   * (32,64,128,256), 3x3 stride-2 VALID convs + ReLU, average pool, Dense(256)+LayerNorm+tanh), gradients of the
   * critic loss flow into its conv kernels */
  int encoder_type;
  int critic_subsample_size; /* sac.py:150-161: 0 = 2 (utils/launcher.py), -1 = None (minimum over all members), else 1..16 */
  int backup_entropy;        /* sac.py:174-176: target_q -= alpha * log pi(a'|s') */
  int tx_lr_set[3];          /* != 0: tx_lr[t] was given explicitly and is honoured even when it is 0 */
  /* T, frames per observation (0 = 1; at most 4).  EncodingWrapper(enable_stacking=True) folds a stack into the channels
   * (common/encoding.py:39-44,58-64: "B T H W C -> B H W (T C)", "B T S -> B (T S)"), so the SmallEncoder's first kernel is
   * (3,3,3T,32) with input channel t*3 + c = channel c of frame t, and state_dim above is the FLATTENED width T * S.
   * T > 1 is served for SERL_ENCODER_SMALL only: the pretrained ResNet-10's conv_init kernel is (7,7,3,64) and cannot be
   * applied to 3T channels (SERL_ERR_UNSUPPORTED). */
  int num_stack;
} serl_agent_cfg;
#define SERL_STD_EXP 0
#define SERL_STD_SOFTPLUS 1
#define SERL_STD_UNIFORM 2
#define SERL_STD_FIXED 3   /* serl_agent_create_opts and serl_agent_create_fixed_std alone */
#define SERL_ACT_TANH 0
#define SERL_ACT_RELU 1
#define SERL_ACT_SWISH 2
#define SERL_ENCODER_RESNET_PRETRAINED 0
#define SERL_ENCODER_SMALL 1
#define SERL_TX_ACTOR 0
#define SERL_TX_CRITIC 1
#define SERL_TX_TEMPERATURE 2

/* LIVE TRUNK.  An agent with SERL_ENCODER_RESNET_PRETRAINED and any tx_weight_decay_on is created in live-trunk mode, because that
 * is what the reference computes (not a recommendation: decaying a pretrained trunk is rarely what a user wants).  Every
 * optimizer step then multiplies every trunk leaf by 1 - sum_t lr_t(count) * wd_t over all three optimizers, whichever networks
 * the step updates, and the target copy follows by the EMA on critic steps only: the online and the target trunk differ from
 * the second step on.  The target critic's encoder reads next-frame features of the TARGET trunk (sac.py:143-147), everything
 * else the online trunk's, and the features are recomputed after every step that changed the trunk: per minibatch inside
 * serl_agent_update_high_utd, and once more before its actor phase.  In this mode the trunk passes run on the stream of the
 * phase that needs them (serl_agent_critic_grads / serl_agent_actor_grads compute what is missing or stale); serl_agent_encode_slot
 * only binds the batch, so a pass cannot run ahead of the step before it, and one slot is all a caller can use.
 * serl_agent_bind_slot / serl_agent_slot_features (features from another GPU) are SERL_ERR_UNSUPPORTED, and reward labels
 * always come from the classifier's own trunk (SERL_LABEL_FRAMES).  Agents without weight decay, and agents without the
 * pretrained trunk (SERL_ENCODER_SMALL, state-only: their decay is the ordinary path of their leaves), are not in this mode and
 * launch what they always did. */
/* NETWORK OPTIONS.  What the critic's and the policy's networks are, beyond serl_agent_cfg, stated once.  Every field is chosen so
 * that 0 means what utils/launcher.py configures: an all-zero serl_agent_opts is serl_agent_create(cfg), and such an agent
 * launches the kernels it always launched.  A value outside what is listed is SERL_ERR_INVALID, the message naming the field and
 * the value.  No option owns a parameter of its own except where said: leaves, optimizer state and checkpoints are otherwise alike.
 * serl_mlp_opts, one per network (networks/mlp.py:19-31; sac.py:516-524 and drq.py:188-207 build the two from separate kwargs, so
 * the two are independent):
 *   act            `activations`, behind every layer: SERL_ACT_TANH y = tanh(p); SERL_ACT_RELU y = max(p, 0), gradient 0 at p = 0
 *                  (jax.nn.relu); SERL_ACT_SWISH y = p * sigmoid(p) (flax.linen.swish = silu, mlp.py's own default).  The encoder's
 *                  bottleneck and proprio rows keep tanh and their LayerNorm (resnet_v1.py:371-374, encoding.py:66-68).
 *   n_layers, dims `hidden_dims`: 1 to SERL_MAX_MLP_LAYERS widths, each a multiple of 64 in [64, 1024] (any integer in [1, 1024] with
 *                  serl_agent_opts.ragged_widths, below, which holds for cfg->hidden too); n_layers == 0 means two
 *                  layers of cfg->hidden, which is read for such a network alone.  Leaves: critic/w<j>, critic/b<j>,
 *                  critic/ln<j>/{scale,bias}, j = 1..n_layers, and the same under actor/; critic/head/kernel follows the critic's
 *                  last width, actor/mean/kernel and actor/logstd/kernel the policy's.
 *   no_layer_norm  1 = `use_layer_norm=False` (mlp.py:29-30; mlp.py's own default, plain SAC and REDQ): every layer is
 *                  y = act(Dense(x) + b) and owns w<j> and b<j> alone -- no ln<j>/{scale,bias} leaf, moment, target copy or
 *                  checkpoint entry; a plain layer takes the place of its LayerNorm launch one for one.
 *   dropout        `dropout_rate` in [0, 1) (mlp.py:27-28: Dense -> Dropout -> LayerNorm -> activation; sac.py:137-176,197-207 run
 *                  every loss with train=True; a positive critic rate is Dropout-Q).  A double, as the reference's is: the keep
 *                  probability is float32(1.0 - rate), rounded once.  A kept element of the Dense output (bias included) is divided
 *                  by it, a dropped one is 0, and the LayerNorm's statistics are those of the masked row; all ensemble members of
 *                  one critic forward drop the SAME elements (one keep-mask [rows][hidden] per (forward, layer)).  The update's
 *                  six MLP evaluations draw (serl_mlp_noise below); serl_agent_sample_actions, serl_agent_eval_q and
 *                  serl_agent_eval_policy are train=False and ignore the rates.  Served with a positive rate in either network:
 *                  n_layers == 0 and no_layer_norm == 0 in BOTH networks (the masks are laid out for two layers of cfg->hidden)
 *                  and a std_param other than SERL_STD_FIXED.
 * serl_agent_opts (actor_critic_nets.py:167-227):
 *   std_param      SERL_STD_EXP      std = clip(exp(Dense_1(h)), std_min, std_max)
 *                  SERL_STD_SOFTPLUS std = clip(softplus(Dense_1(h)), std_min, std_max)
 *                  SERL_STD_UNIFORM  std = clip(exp(log_stds), std_min, std_max): one trainable vector of act_dim floats shared by
 *                                    all rows, leaf actor/log_stds in place of actor/logstd/{kernel,bias} (create_drq's own default)
 *                  SERL_STD_FIXED    std = clip(fixed_std, std_min, std_max), the same for every row, in float32 inside the head
 *                                    kernels (:189-192,212, how the reference writes TD3).  The head then has NO std parameter: no
 *                                    actor/logstd/{kernel,bias} and no actor/log_stds leaf, one head GEMM group (the mean), and no
 *                                    gradient, moment, target copy or checkpoint entry for a std.  With the tanh bijector log pi
 *                                    still depends on the mean through the log-determinant; with no_tanh == 1 it depends on no
 *                                    parameter and the actor gradient is dL/da alone.
 *   no_tanh        0 = distrax Tanh bijector on the Gaussian; 1 = tanh_squash_distribution=False: the plain Gaussian -- actions are
 *                  unbounded, log pi has no log-det term, and the mode is the mean
 *   fixed_std      act_dim floats (host memory, copied), each finite and > 0, with SERL_STD_FIXED; NULL with every other
 *                  std_param.  A constant of the agent: device memory of its own outside the parameter arena, never stepped,
 *                  averaged or all-reduced, and not part of serl_agent_get / serl_agent_set (serl_agent_fixed_std reads it back).
 *   ragged_widths  0: every MLP width (dims[], cfg->hidden) is a multiple of 64 in [64, 1024], checked and refused as always.
 *                  1: every width is any integer in [1, 1024] (mlp.py:19-31 takes any list; TD3's and DDPG's published [400, 300]).
 *                  A layer of true width d is STORED dp = 64 * ceil(d / 64) wide: the columns [d, dp) of w<j>, b<j> and
 *                  ln<j>/{scale,bias}, and the rows [d, dp) of the kernel that reads the layer (w<j+1>, critic/head/kernel,
 *                  actor/mean/kernel, actor/logstd/kernel) are padding, exactly 0.0f in the parameters, the target parameters, the
 *                  Adam moments and the gradients, after any sequence of calls (debug tap "pad_max_abs").  The update launches
 *                  what the agent of widths dp launches; only the LayerNorm rows of a layer off the grid are instantiations of
 *                  their own, which divide by d.  serl_agent_leaf_info, serl_agent_set, serl_agent_get and serl_agent_mlp_dims
 *                  speak of true extents alone and never touch padding; what exposes storage says so below
 *                  (serl_agent_leaf_layout).  An agent whose widths all lie on the grid is the agent of ragged_widths 0, bit for
 *                  bit.  A positive dropout beside any width off the grid is refused (the keep-masks are laid out for widths on
 *                  the grid).  The entry points from before serl_agent_opts leave it 0.
 *   no_proprio     0: EncodingWrapper(use_proprio=True), the agent as it always was.  1: use_proprio=False (common/encoding.py:53-72;
 *                  the reference's own default in create_drq): the code is the concatenated camera codes alone, E = bottleneck *
 *                  n_cam, critic/w1 has E + act_dim rows and actor/w1 E.  There is NO enc/proprio/... leaf, moment, target copy,
 *                  gradient, snapshot or checkpoint entry, and no proprio scratch.  The state is never read: serl_batch.state and
 *                  every dev_state argument may be NULL; cfg->state_dim is validated (>= 1) and matched against serl_batch as
 *                  always, and otherwise unused; cfg->proprio_dim must still be 64 and is ignored.  An update launches no proprio
 *                  rows and no kernel that does proprio work only; the actions rider of the encoder pass (the batch's actions into
 *                  the critic input [enc | action]) rides on the SpatialLearnedEmbeddings launch as trailing workgroups where that
 *                  launch carried the proprio rows, and is one column-copy launch where the proprio rows were a launch of their
 *                  own.  n_cam == 0 with no_proprio 1 is SERL_ERR_INVALID (a state-only agent has no EncodingWrapper); a positive
 *                  dropout in either MLP beside no_proprio 1 is SERL_ERR_UNSUPPORTED.  Any other value is SERL_ERR_INVALID.  The
 *                  entry points from before serl_agent_opts leave it 0. */
#define SERL_MAX_MLP_LAYERS 4
typedef struct serl_mlp_opts {
  int act;
  int n_layers;
  int dims[SERL_MAX_MLP_LAYERS];
  int no_layer_norm;
  double dropout;
} serl_mlp_opts;
typedef struct serl_agent_opts {
  int std_param;
  int no_tanh;
  serl_mlp_opts critic, policy;
  const float* fixed_std;
  int ragged_widths;
  int no_proprio;
} serl_agent_opts;
int serl_agent_create_opts(const serl_agent_cfg* cfg, const serl_agent_opts* opts, serl_agent** out);
int serl_agent_live_trunk(serl_agent* a);   /* 1: live-trunk mode (above), 0: not, -1: NULL */
int serl_agent_use_proprio(serl_agent* a);  /* 1: the agent has the proprio branch, 0: no_proprio (above), -1: NULL */
/* The entry points from before serl_agent_opts: each sets the fields its arguments name and leaves the others 0.  The three that
 * take the width lists refuse a NULL list and never read cfg->hidden; all but serl_agent_create_fixed_std refuse SERL_STD_FIXED. */
int serl_agent_create(const serl_agent_cfg* cfg, serl_agent** out);   /* no field: the all-zero opts */
int serl_agent_create_policy(const serl_agent_cfg* cfg, int std_param, int no_tanh, serl_agent** out);   /* std_param, no_tanh */
int serl_agent_create_mlp(const serl_agent_cfg* cfg, int std_param, int no_tanh, int critic_act, int policy_act, serl_agent** out);   /* ... and both act */
/* ... and both dropout */
int serl_agent_create_dropout(const serl_agent_cfg* cfg, int std_param, int no_tanh, int critic_act, int policy_act,
                              double critic_dropout, double policy_dropout, serl_agent** out);
/* serl_agent_create_mlp's fields and both n_layers / dims */
int serl_agent_create_shapes(const serl_agent_cfg* cfg, int std_param, int no_tanh, int critic_act, int policy_act,
                             const int* critic_dims, int n_critic, const int* policy_dims, int n_policy, serl_agent** out);
/* ... and both no_layer_norm, as its complement: critic_layer_norm / policy_layer_norm 1 = LayerNorm, 0 = none */
int serl_agent_create_layer_norm(const serl_agent_cfg* cfg, int std_param, int no_tanh, int critic_act, int policy_act,
                                 const int* critic_dims, int n_critic, const int* policy_dims, int n_policy, int critic_layer_norm,
                                 int policy_layer_norm, serl_agent** out);
/* ... and fixed_std, with std_param up to SERL_STD_FIXED */
int serl_agent_create_fixed_std(const serl_agent_cfg* cfg, int std_param, int no_tanh, int critic_act, int policy_act,
                                const int* critic_dims, int n_critic, const int* policy_dims, int n_policy, int critic_layer_norm,
                                int policy_layer_norm, const float* fixed_std, serl_agent** out);
/* The hidden widths of one MLP of any agent (networks/mlp.py:19-31; sac.py:516-524, drq.py:188-207): network 0 = critic,
 * 1 = policy.  Returns the layer count and fills dims[0 .. count); -1 on a NULL argument or another network code. */
int serl_agent_mlp_dims(serl_agent* a, int network /* 0 critic, 1 policy */, int dims[SERL_MAX_MLP_LAYERS]);  /* -> layer count */
/* Whether the layers of one MLP of any agent have their LayerNorm (networks/mlp.py:29-30): network 0 = critic, 1 = policy.
 * Returns 1 or 0; -1 on a NULL agent or another network code. */
int serl_agent_mlp_layer_norm(serl_agent* a, int network /* 0 critic, 1 policy */);
/* The fixed_std vector of an agent made with SERL_STD_FIXED, as passed (before the clip): out = act_dim floats (host).
 * SERL_ERR_INVALID on a NULL argument or an agent of another std parameterisation. */
int serl_agent_fixed_std(serl_agent* a, float* out);
int serl_agent_destroy(serl_agent* a);

/* Parameter tree access (flat leaf names, see DESIGN.md "parameter arena"; the Python shim maps
 * them to the flax tree of agent.state.params for publish_network / checkpoints).
 * section: "params" | "target_params" | "opt/<tx>/mu" | "opt/<tx>/nu", tx in actor|critic|temperature */
int serl_agent_num_leaves(serl_agent* a);
int serl_agent_leaf_info(serl_agent* a, int i, char* name_out, int name_cap, int64_t* count);
int serl_agent_set(serl_agent* a, const char* section, const char* leaf, const float* host, int64_t count);
int serl_agent_get(serl_agent* a, const char* section, const char* leaf, float* host_out, int64_t count);
/* How a leaf is stored (ragged_widths above): out = {n, rows, cols, rows_p, ld}.  The leaf is n blocks of rows x cols elements --
 * n * rows * cols is serl_agent_leaf_info's count, and the order of serl_agent_get's elements -- inside n blocks of rows_p x ld
 * floats: element (i, r, c) is float (i * rows_p + r) * ld + c of the leaf's storage, and every other float of the n * rows_p * ld
 * is padding, exactly 0.  A leaf without padding reports rows_p == rows and ld == cols, or {1, 1, count, 1, count}.  For readers
 * of what exposes storage: serl_agent_grad_view and serl_agent_grad_bucket (the gradient of a leaf lies where the leaf lies, padding
 * included; an all-reduce over the whole range keeps the padding zero) and serl_snapshot_leaf (which returns the storage). */
int serl_agent_leaf_layout(serl_agent* a, const char* leaf, int64_t out[5]);
int serl_agent_set_step(serl_agent* a, int64_t step); /* JaxRLTrainState.step and the Adam counts */
/* Arithmetic of the frozen trunk's 3x3/1x1 convs: 0 = exact fp32 MFMA, 1 (default) = split-fp16
 * ("f16x3": x = hi + 2^-11 lo', three fp16 MFMA products per fp32 product, fp32 accumulate; error per
 * product <= ~3*2^-22, i.e. fp32-roundoff class -- DESIGN.md section 4; parity tests run both modes). */
int serl_agent_set_trunk_mode(serl_agent* a, int mode);
/* Scheduling hint (results equal up to fp32 summation order: the K-split depth sets how many partial sums a GEMM adds;
 * per agent, read by that agent's launches only): the most workgroups a K-split GEMM launch of the update (sac.py:243-299) may use
 * (0 = default 512).  A caller that overlaps the update of batch i with the frozen-trunk pass of batch i+1 at a large per-rank
 * batch sets 256: fewer update workgroups queue for CU slots between the trunk's conv workgroups. */
int serl_agent_set_chain_budget(serl_agent* a, int workgroups);
int64_t serl_agent_get_step(serl_agent* a);

/* Parameter snapshots (csrc/snapshot.hip).  The reference's learner sends its parameters to the actor every 30 iterations and
 * writes a checkpoint every few thousand (examples/async_drq_sim/async_drq_sim.py:229,295-307); serl_agent_get serves that with one
 * blocking copy per leaf.  A serl_snapshot handle takes a CONSISTENT copy of the selected sections in one kernel launch on the
 * update stream and moves it to pinned host memory on a stream of its own: what was enqueued on `stream` before the take is in
 * the snapshot, what is enqueued after it is not and may start as soon as the pack kernel is done.
 *   sections  SERL_SNAP_PARAMS | SERL_SNAP_TARGET | SERL_SNAP_OPT: "params", "target_params", and "opt/<tx>/mu" + "opt/<tx>/nu"
 *             of the three optimizers.  A moment outside its optimizer's support reads as zeros, as with serl_agent_get.
 *   slots     1..4 snapshots that can be held at once.  A slot is held from take until release.
 * take / ready / wait / info / leaf / release may be called from any thread (slot states sit behind a mutex in the handle; take
 * never waits for a reader).  create and destroy belong to the thread that owns the agent, like every serl_agent_* call (the
 * agent's count of live handles is not locked), and destroy must not run while another thread is inside a call on the handle.
 * SERL_ERR_STATE: take with every slot held -- or released while its copy to the host was still running, a slot is never
 * overwritten under a copy -- or with a stream of another device (nothing is enqueued then); info / leaf before the slot's copy
 * is complete; any call on a slot that holds nothing.
 * An agent with a live snapshot handle cannot be destroyed: serl_agent_destroy returns SERL_ERR_STATE and leaves the agent as it
 * was; destroy the snapshot handles first. */
typedef struct serl_snapshot serl_snapshot;
#define SERL_SNAP_PARAMS 1
#define SERL_SNAP_TARGET 2
#define SERL_SNAP_OPT 4
typedef struct serl_snapshot_meta {
  int64_t step;          /* serl_agent_get_step at the take */
  int64_t trunk_gen;     /* trunk leaves set on the agent up to the take */
  int64_t bytes;         /* bytes one take copies to the host (header + every contiguous run, each padded to 16 bytes) */
  int64_t nonfinite[3];  /* Inf / NaN values found while packing, per section: [params, target_params, opt] (0 where not selected) */
  int sections, slots;   /* as created */
} serl_snapshot_meta;
/* async_drq_sim.py:229,295-307.  Resolves every (section, leaf) once, merges the device ranges into their maximal contiguous runs
 * and allocates, per slot, a device staging buffer and its pinned host twin; one copy stream and two events per slot. */
int serl_snapshot_create(serl_agent* a, int sections, int slots, serl_snapshot** out);
/* async_drq_sim.py:295-297,303-307.  Returns without waiting for the device.  On `stream` (the stream the agent's updates run
 * on): a memset of the slot's counters, ONE snapshot_pack_kernel launch, an event; on the handle's copy stream: a wait on that
 * event, one copy of the whole slot to its pinned buffer, a second event.  *slot_out is the slot now held. */
int serl_snapshot_take(serl_snapshot* s, void* stream, int* slot_out);
/* async_drq_sim.py:295-297.  1 = the slot's copy is complete, 0 = not yet (never blocks), negative = status. */
int serl_snapshot_ready(serl_snapshot* s, int slot);
/* async_drq_sim.py:295-297.  Blocks the calling thread (not the device, and no other thread's take) until the copy is complete. */
int serl_snapshot_wait(serl_snapshot* s, int slot);
/* async_drq_sim.py:295-307.  What the slot holds; refused before its copy is complete. */
int serl_snapshot_info(serl_snapshot* s, int slot, serl_snapshot_meta* out);
/* async_drq_sim.py:229,295-307.  *host_out points INTO the slot's pinned buffer (read-only for the caller; shared zeros for a
 * moment outside its optimizer's support) and is valid until serl_snapshot_release; refused before the copy is complete. */
/* The pack kernel copies contiguous runs: a leaf stored with padding (serl_agent_leaf_layout) arrives as its storage, *count is
 * n * rows_p * ld, and the caller cuts the leaf's own elements out of it. */
int serl_snapshot_leaf(serl_snapshot* s, int slot, const char* section, const char* leaf, const float** host_out, int64_t* count);
/* async_drq_sim.py:295-307.  The slot may be taken again (once its copy, if still running, has ended). */
int serl_snapshot_release(serl_snapshot* s, int slot);
/* async_drq_sim.py:295-307.  Waits for what the handle has in flight, frees it; the agent can be destroyed again. */
int serl_snapshot_destroy(serl_snapshot* s);

/* Explicit randomness (parity mode).  All pointers are DEVICE addresses; NULL members (or a NULL
 * struct) are generated on the device from cfg.seed.  Shapes use the batch of the call:
 *   eps_*  f32[batch][act_dim];  mask_* u8[n_cam][batch][512*sle_features] keep-masks (1 = keep)
 * redq_idx is a HOST pointer: int32[utd_ratio][critic_subsample_size] (sac.py:150-157; unused when the size is None). */
typedef struct serl_noise {
  const float* eps_next;          /* critic loss: policy sample at next_obs (sac.py:118-132) */
  const uint8_t* mask_next;       /* Dropout(0.1) masks of that policy forward */
  const int32_t* redq_idx;        /* host */
  const float* eps_pi;            /* policy loss sample at obs (sac.py:197-201) */
  const uint8_t* mask_obs_pi;
  const float* eps_temp;          /* temperature loss sample at next_obs (sac.py:224-227) */
  const uint8_t* mask_next_temp;
  /* Round 5 -- jax.random KEYS instead of tensors (HOST pointers to uint32 words; NULL = none).  Where the tensor above is NULL
   * and its key is given, the draws are jax.random's for that key (serl_jax_* below: bits exact, normals through XLA's float32
   * erf_inv), produced INSIDE the kernels that consume them -- no noise tensor exists, no extra launch.  Array shapes are the
   * reference's: normal(key, (global minibatch rows, act_dim)), bernoulli(key_cam, 1 - dropout, (global minibatch rows, 4096));
   * a rank of a data-parallel job draws its rows of them (serl_agent_set_shard).  key_*_next are indexed by the minibatch of a
   * high-UTD update (redq_row): [utd][2] and [utd][n_cam][2]; the others are [2] and [n_cam][2]. */
  const uint32_t* key_eps_next;
  const uint32_t* key_mask_next;
  const uint32_t* key_eps_pi;
  const uint32_t* key_mask_obs_pi;
  const uint32_t* key_eps_temp;
  const uint32_t* key_mask_next_temp;
} serl_noise;

/* The MLP Dropout draws of an agent made by serl_agent_create_dropout (mlp.py:27-28; sac.py:137-176,197-207).  serl_noise is
 * unchanged; this struct is BOUND to the agent and consumed by the next update / phase / dry-run call (serl_agent_update*,
 * serl_agent_critic_grads*, serl_agent_actor_grads, serl_agent_eval_losses): that call reads it -- an update reads it in all of
 * its phases -- and the binding is gone when it returns.  Six evaluations ("sites") draw, each in both hidden layers:
 *   SERL_SITE_PI_NEXT   policy at next_obs inside the critic loss      (policy rate; one draw per critic update)
 *   SERL_SITE_Q_TARGET  target critic at next_obs                      (critic rate; one draw per critic update)
 *   SERL_SITE_Q_ONLINE  online critic at obs                           (critic rate; one draw per critic update)
 *   SERL_SITE_PI        policy at obs inside the actor loss            (policy rate)
 *   SERL_SITE_Q_ACTOR   critic at obs inside the actor loss            (critic rate)
 *   SERL_SITE_PI_TEMP   policy at next_obs inside the temperature loss (policy rate)
 * Per site, in this order of preference:
 *   mask[site]  DEVICE u8 keep-masks [2 layers][batch][hidden], 1 = keep, batch = the rows of the call's batch; the critic-loss
 *               sites of minibatch i of a high-UTD update read the rows of that minibatch.
 *   key[site]   HOST uint32 words: per layer the key of jax.random.bernoulli(key, 1 - rate, (global minibatch rows, hidden)), drawn
 *               inside the LayerNorm rows (a data-parallel rank draws its rows of it, serl_agent_set_shard) -- flax's make_rng at
 *               the Dropout layer's scope path.  Critic-loss sites: [utd][2 layers][2], indexed by redq_row; the others [2 layers][2].
 *   neither     hashed on the device from cfg.seed, a stream per (site, layer) indexed by the global row: the ranks of a
 *               data-parallel job agree.  The hash gives the target and the online critic independent masks also where the
 *               reference, with critic_subsample_size None, would give them the same one.
 * A site whose network has rate 0 reads nothing.  serl_agent_set_mlp_noise(a, NULL) clears a binding. */
enum { SERL_SITE_PI_NEXT = 0, SERL_SITE_Q_TARGET = 1, SERL_SITE_Q_ONLINE = 2, SERL_SITE_PI = 3, SERL_SITE_Q_ACTOR = 4, SERL_SITE_PI_TEMP = 5,
       SERL_MLP_SITES = 6 };
typedef struct serl_mlp_noise {
  const uint8_t* mask[SERL_MLP_SITES];
  const uint32_t* key[SERL_MLP_SITES];
  int32_t mask_rows;   /* `batch` of the mask tensors: a call on a batch of another size is refused (SERL_ERR_INVALID) */
} serl_mlp_noise;
int serl_agent_set_mlp_noise(serl_agent* a, const serl_mlp_noise* noise);

/* sac.py:185-189,215-219,234,291-297 */
typedef struct serl_info {
  float critic_loss, predicted_qs, target_qs;
  float actor_loss, temperature, entropy, temperature_loss;
  float actor_lr, critic_lr, temperature_lr;
} serl_info;

/* DrQAgent.update_critics (drq.py:296-328) on an augmented device batch: one critic grad-step
 * (REDQ target, 10-member ensemble MSE), 3x Adam (actor/temperature with zero gradients), target EMA. */
int serl_agent_update_critics(serl_agent* a, const serl_batch* batch, const serl_noise* noise, void* stream);
/* DrQAgent.update_high_utd (drq.py:255-294 -> sac.py:544-596): utd_ratio critic updates on
 * consecutive minibatches, then one actor + temperature update on the full batch. */
int serl_agent_update_high_utd(serl_agent* a, const serl_batch* batch, int utd_ratio,
                               const serl_noise* noise, void* stream);
/* info of the last update call (synchronises `stream`) */
int serl_agent_read_info(serl_agent* a, serl_info* host_out, void* stream);

/* Data-parallel phases (common.py:213-214 lax.pmean made real).  Rank r holds samples
 * [r*B/P,(r+1)*B/P) of the global batch; the caller all-reduces (SUM) the gradient view between
 * *_grads and apply.  global_count = samples of this (mini)batch over all ranks (loss normaliser). */
int serl_agent_encode(serl_agent* a, const serl_batch* batch, void* stream); /* frozen trunk, both passes */
/* Software pipelining: the frozen trunk does not depend on the trainable parameters, so the trunk
 * pass of batch i+1 (another slot, on a second stream) may overlap the update of batch i.  There are
 * THREE slots (0..2): with two, the pass of batch i+2 has to wait ON THE DEVICE for the update of batch i
 * (a cross-stream dependency, 60-100 us on this stack); with three it reuses the slot of batch i-1, whose
 * update a host that runs one step ahead can confirm with an event query.  The caller orders the
 * streams with events; serl_agent_select_slot picks the batch the following *_grads calls consume.
 * serl_agent_encode == encode_slot(0) + select_slot(0). */
int serl_agent_encode_slot(serl_agent* a, const serl_batch* batch, int slot, void* stream);
/* The same pass issued in consecutive pieces: stages [stage_begin, stage_end] with -1 = conv_init + max-pool and 0..3 = the
 * residual stages (split-fp16 trunk, full-size batch).  The caller may record an event between two pieces, e.g. to start
 * the update of the previous batch only once this pass has left its first stages. */
int serl_agent_encode_slot_range(serl_agent* a, const serl_batch* batch, int slot, int stage_begin, int stage_end, void* stream);
int serl_agent_select_slot(serl_agent* a, int slot);
/* Features computed ELSEWHERE.  The trunk is frozen and its output is cut off by a stop_gradient (vision/resnet_v1.py:286), so
 * the features of a batch depend on its pixels only -- another GPU can run that pass ("trunk farm": serl_amd/parallel.py
 * TrunkFarmLearner).  serl_agent_slot_features gives the slot's feature buffer f32[2][n_cam][batch][h*w][512] (what encode_slot
 * writes; a producer sends from it, the updating rank receives into it); serl_agent_bind_slot attaches a batch (states, actions,
 * rewards, masks -- and its frames, which the update does not read) to a slot WITHOUT running the trunk. */
int serl_agent_slot_features(serl_agent* a, int slot, float** dev_out, int64_t* count_out);
int serl_agent_bind_slot(serl_agent* a, const serl_batch* batch, int slot);
int serl_agent_critic_grads(serl_agent* a, int offset, int count, int global_count,
                            const serl_noise* noise, int redq_row, void* stream);
/* The same critic phase with its gradients published in two BUCKETS so the caller can all-reduce the first while the
 * second is still being computed (the pmean of common.py:213-214 overlapped with the backward pass, as DDP-style bucketing
 * does): `event_bucket0` (a hipEvent_t, may be NULL) is recorded on `stream` as soon as bucket 0 is final -- before the
 * encoder-head backward (Dense 4096->256 weight gradient, SpatialLearnedEmbeddings / SmallEncoder gradients) is issued.
 *   bucket 0 = [critic ensemble | Q head | proprio branch | loss scalars]   (contiguous; ~8.7 MB at the headline shape)
 *   bucket 1 = [per-camera encoder heads]                                    (contiguous; ~8.9 MB; empty for state-only SAC)
 * Both are final when the call's work on `stream` has completed.  serl_agent_grad_bucket returns their device ranges. */
int serl_agent_critic_grads_bucketed(serl_agent* a, int offset, int count, int global_count, const serl_noise* noise,
                                     int redq_row, void* stream, void* event_bucket0);
int serl_agent_grad_bucket(serl_agent* a, int bucket, float** dev_ptr, int64_t* count);
int serl_agent_actor_grads(serl_agent* a, int global_count, const serl_noise* noise, void* stream);
/* `which` = networks_to_update of SACAgent.update (sac.py:243-299) as a bit set; optimizers whose bit is clear still
 * step with a zero gradient (sac.py:276-277).  The target EMA runs iff SERL_NET_CRITIC is set (sac.py:284-285). */
#define SERL_NET_CRITIC 1
#define SERL_NET_ACTOR 2
#define SERL_NET_TEMPERATURE 4
#define SERL_APPLY_CRITIC SERL_NET_CRITIC
#define SERL_APPLY_ACTOR_TEMP (SERL_NET_ACTOR | SERL_NET_TEMPERATURE)
int serl_agent_apply(serl_agent* a, int which, float info_weight, void* stream);
/* SACAgent.update(batch, networks_to_update) (sac.py:243-299) on an augmented device batch: every selected loss is
 * evaluated at the SAME (pre-update) parameters, then ONE optimizer step of all three Adam transforms (+ target EMA
 * if the critic is selected).  nets = any non-empty combination of SERL_NET_*. */
int serl_agent_update(serl_agent* a, const serl_batch* batch, int nets, const serl_noise* noise, void* stream);
int serl_agent_begin_update(serl_agent* a, void* stream); /* clears the info accumulator */
/* Batch-sharded data parallelism: the batches this agent is given are rows [global_offset, global_offset + local
 * batch) of a global batch of `global_batch` rows.  Device-generated noise (noise == NULL) is then indexed by the
 * GLOBAL row, so a sample gets the same eps / dropout mask whichever rank owns it and results do not depend on the
 * world size (the dormant pmean of common.py:213-214 made real).  global_batch = 0: not sharded (default). */
int serl_agent_set_shard(serl_agent* a, int64_t global_offset, int64_t global_batch);
/* which = SERL_APPLY_CRITIC: [critic grads | scalars]; SERL_APPLY_ACTOR_TEMP (or any actor/temperature bit):
 * [scalars | actor grads]; critic AND actor/temperature bits: the whole [critic grads | scalars | actor grads] range */
int serl_agent_grad_view(serl_agent* a, int which, float** dev_ptr, int64_t* count);

/* SACAgent.sample_actions (sac.py:301-320): policy forward with train=False on `n` observations
 * (frames u8[n_cam][n][T][H][W][3], state f32[n][T*S], both device; T = cfg.num_stack); eps f32[n][A] device or NULL for
 * argmax (= distribution mode).  out_actions f32[n][A] device. */
int serl_agent_sample_actions(serl_agent* a, const uint8_t* dev_frames, const float* dev_state, int n,
                              const float* dev_eps, float* dev_out_actions, void* stream);

/* ---- Read-only evaluation: what the trained networks think, without a step -------------------------------------------------
 * The three entries below read the parameters and leave every piece of training state as it was: no byte of the online or
 * target parameters, the Adam moments, the step counter, the agent's noise counter, the reward-label state, or the three
 * pipeline slots (their trunk features and batch bindings) is written.  They use the scratch feature slot of
 * serl_agent_sample_actions, the activations, the gradient scratch and an info accumulator of their own; the next update
 * starts with serl_agent_begin_update as always.  They share the trunk workspace with serl_agent_encode_slot: order them
 * behind a trunk pass in flight on another stream, as for serl_agent_sample_actions.  No Dropout (train=False) in the first two.
 * Refused with SERL_ERR_INVALID, the message naming the argument and the value: n outside [1, cfg.batch]; dev_logp_out without
 * dev_actions; NULL dev_frames on an agent with cameras (a state-only agent, n_cam == 0, takes NULL). */
/* forward_critic(obs, actions, train=False) (sac.py:33-55); target != 0: with target_params (sac.py:57-69).
 * frames u8[n_cam][n][T][H][W][3], state f32[n][T*S], actions f32[n][A], all device, 1 <= n <= cfg.batch;
 * q_out f32[ensemble][n] device. */
int serl_agent_eval_q(serl_agent* a, const uint8_t* dev_frames, const float* dev_state, const float* dev_actions,
                      int n, int target, float* dev_q_out, void* stream);
/* forward_policy(obs, train=False) (sac.py:71-91): loc, scale_diag, mode, and log_prob(dev_actions) when given.
 * Any output pointer may be NULL; dev_logp_out requires dev_actions.  mean, std, mode f32[n][A], logp f32[n], device.
 * Under the tanh squash log_prob follows distrax's Transformed.log_prob with the Tanh bijector: u = atanh(a),
 * sum_j [log N(u_j; loc_j, scale_j) - 2 (log 2 - u_j - softplus(-2 u_j))]; without it, the diagonal Gaussian's log-density.
 * An action component with |a| >= 1 has no finite atanh: that row's log_prob is not finite, here as in the reference, and is
 * NOT clamped -- stored gripper commands of exactly +-1 are common; clip them to the open interval before asking. */
int serl_agent_eval_policy(serl_agent* a, const uint8_t* dev_frames, const float* dev_state, const float* dev_actions,
                           int n, float* dev_mean_out, float* dev_std_out, float* dev_mode_out, float* dev_logp_out,
                           void* stream);
/* loss_fns(batch) evaluated, not applied (sac.py:134-241): the critic, actor and temperature phases of
 * serl_agent_update on `batch` with `noise`, WITHOUT serl_agent_apply.  host_out gets the seven loss scalars and the
 * three learning rates an update at the current step would report (synchronises `stream`).  The scalars are bit for bit those
 * of the serl_agent_update(batch, all three networks, noise) that follows; like that call it keeps the stored rewards when a
 * reward classifier is attached. */
int serl_agent_eval_losses(serl_agent* a, const serl_batch* batch, const serl_noise* noise, serl_info* host_out, void* stream);

/* Debug / test taps (device->host copies of internal activations). */
int serl_agent_trunk_forward(serl_agent* a, const uint8_t* dev_frames, int n, float* dev_feats_out, void* stream);
/* "pad_max_abs" (one value, read-only): the largest |value| over all padding of the ragged layout (ragged_widths).  Covered: every
 * leaf whose storage is larger than its element count (serl_agent_leaf_layout: n * rows_p * ld > n * rows * cols) -- pad columns
 * [cols, ld) of every row and pad rows [rows, rows_p) of every block, those of the one-block kernels actor/mean/kernel,
 * actor/logstd/kernel and actor/w<j> included -- in the parameters, the target parameters, both Adam moments of the critic's and
 * of the actor's optimizer and both gradient buffers.  Not covered: the temperature's moments and the trunk (neither has
 * padding).  The layout's invariant is that it reads exactly 0 (NaN reads as infinity; 0 for an agent without padding).  The MLP taps
 * ("mlp_xhat/...", "mlp_dpre/...") hold rows of the storage width. */
int serl_agent_debug_get(serl_agent* a, const char* what, float* host_out, int64_t count);
/* inject gradients / scalars ("g_critic", "g_actor", "scalars") before serl_agent_apply: optimizer tests */
int serl_agent_debug_set(serl_agent* a, const char* what, const float* host, int64_t count);
/* Which kernels the LAST split-fp16 trunk pass selected, as text ("images=128 pool=1 raw_b0=0 b0_conv0=S/1/0/f1/p1x1 ...":
 * layer=kernel/tile-config/statistics-mode/f<fused epilogue>/p<low-side SAME pad of the rows>x<of the columns>; kernel S =
 * row-slab, D = LDS-DMA, R = register-staged implicit GEMM, F = projection computed by conv0's launch).  Image extents that
 * are not powers of two pick other pads and kernels than 64 / 128 do, and the per-rank shapes of a data-parallel job
 * (resnet_v1.py:260-269 at N = B/8 images) pick other kernels than the full batch; the parity tests assert which path they
 * exercised.  A buffer the text (about 350 bytes) does not fit in is refused with SERL_ERR_INVALID, never truncated. */
int serl_agent_trunk_plan(serl_agent* a, char* out, int cap);
/* Number of update-chain kernels (everything but the frozen trunk, the SmallEncoder convs and the replay kernels) launched
 * since the library was loaded: the tests pin the launch count of an update_critics + update_high_utd pair (sac.py:243-299). */
int64_t serl_debug_chain_launches(void);

/* ---------------------------------------------------------------------------------------------
 * Reward classifier (next-row N4; serl_launcher/networks/reward_classifier.py:16-113).
 * BinaryClassifier = EncodingWrapper(use_proprio=False) over the frozen ResNet-10 trunk (per camera:
 * SpatialLearnedEmbeddings(8) -> Dense(256) -> LayerNorm -> tanh, concatenated) -> Dense(256) -> [Dropout: identity at
 * train=False] -> LayerNorm -> ReLU -> Dense(1).  serl_classifier_logits is the function load_classifier_func
 * (reward_classifier.py:93-113) returns: observations in, logits out.  Leaves (flat fp32, HWIO kernels / [in][out]
 * dense kernels): the trunk leaves of the agent ("trunk/..."), "enc/<k>/{sle, dense/kernel, dense/bias, ln/scale,
 * ln/bias}", "head/dense0/{kernel,bias}", "head/ln/{scale,bias}", "head/dense1/{kernel,bias}".
 * --------------------------------------------------------------------------------------------- */
typedef struct serl_classifier serl_classifier;
typedef struct {
  int device, n_cam, H, W, max_batch;
} serl_classifier_cfg;
int serl_classifier_create(const serl_classifier_cfg* cfg, serl_classifier** out);
int serl_classifier_destroy(serl_classifier* c);
int serl_classifier_num_leaves(serl_classifier* c);
int serl_classifier_leaf_info(serl_classifier* c, int i, char* name_out, int name_cap, int64_t* count);
int serl_classifier_set(serl_classifier* c, const char* leaf, const float* host, int64_t count);
int serl_classifier_get(serl_classifier* c, const char* leaf, float* host_out, int64_t count);
/* dev_frames u8[n_cam][n][H][W][3] (device), n <= max_batch; dev_logits f32[n] (device) */
int serl_classifier_logits(serl_classifier* c, const uint8_t* dev_frames, int n, float* dev_logits, void* stream);
/* The same logits from frozen-trunk features that already exist (serl_classifier_logits = the trunk, then this): per camera
 * SpatialLearnedEmbeddings -> Dense -> LayerNorm -> tanh, then the head.  Classifier camera k reads the n feature maps
 * f32[n][h*w][512] at dev_feats + cam_of[k] * cam_stride_floats (cam_of: host int[n_cam], any order, entries may
 * repeat; every entry >= 0, and the caller guarantees that each camera it names lies inside the buffer at dev_feats: the
 * function knows neither how many cameras the buffer holds nor its size, and reads where the entry points). */
int serl_classifier_logits_from_features(serl_classifier* c, const float* dev_feats, int64_t cam_stride_floats, const int* cam_of,
                                         int n, float* dev_logits, void* stream);

/* Reward labelling inside the DrQ update: the part of VICEAgent that changes what the critic learns from
 * (agents/continuous/vice.py:546 in update_critics, :594 in update_high_utd):
 *     rewards = (sigmoid(classifier(augmented next_obs, train=False)) >= 0.5) * 1.0
 * computed once per call over the whole batch and used in place of the stored rewards.  SACAgent.update is not overridden by
 * VICE and keeps the stored rewards (serl_agent_update).  mixup, label smoothing and the gradient penalty of update_vice are
 * not built; the classifier is trained by serl_classifier_train_step.
 * serl_agent_set_reward_classifier attaches `c` (NULL detaches).  cam_of: host int[classifier n_cam], the agent camera each
 * classifier camera reads.  Refused: a state-only agent, a camera index the agent lacks, another image size or device, a
 * classifier max_batch below the agent's batch, an agent with num_stack > 1 (the classifier reads single frames).  *mode_out (may be NULL) = SERL_LABEL_FEATURES when the agent has a frozen
 * trunk whose every leaf is bit-identical to the classifier's (compared here, once): the classifier's head then runs on the
 * trunk features of the augmented next observations that the agent's slot already holds; else SERL_LABEL_FRAMES: the
 * classifier's own trunk runs on the batch's augmented next frames.  Both handles count the trunk leaves set on them; a trunk
 * leaf set on either after the attach makes the next labelling fail with SERL_ERR_STATE until the classifier is attached
 * again.  The handle is borrowed: it must outlive the attachment.  Labelling reads the classifier's parameters and uses its
 * scratch on the update's stream; a serl_classifier_train_step or serl_classifier_logits on another stream is the caller's to order. */
#define SERL_LABEL_NONE 0
#define SERL_LABEL_FEATURES 1
#define SERL_LABEL_FRAMES 2
int serl_agent_set_reward_classifier(serl_agent* a, serl_classifier* c, const int* cam_of, int* mode_out);
/* Labels the selected batch (vice.py:594): label[i] = 1 / (1 + expf(-logit_i)) >= 0.5f in fp32, into a buffer of the agent;
 * the critic phases that follow read it instead of the batch's rewards, until another batch is selected.  The batch and the
 * replay store are not written.  serl_agent_update_critics / _update_high_utd call it themselves when a classifier is attached;
 * a phase-API caller does, after serl_agent_select_slot / serl_agent_encode (serl_agent_critic_grads refuses otherwise).  Under
 * serl_agent_set_shard a rank labels its own rows.  No random number is drawn (train=False). */
int serl_agent_label_rewards(serl_agent* a, void* stream);
int serl_agent_reward_label_rows(serl_agent* a);   /* rows of the last labelling (0: none yet) */
/* Labels, logits (host f32[rows of the last labelling], rows <= cfg.batch) and the mean label (vice.py:609 "vice_rewards") of the
 * last labelling; NULL members are skipped.  Synchronises `stream`. */
int serl_agent_read_reward_labels(serl_agent* a, float* host_labels, float* host_logits, float* mean_out, void* stream);

/* Training (examples/async_cable_route_drq/train_reward_classifier.py:122-137; the same file in async_bin_relocation_fwbw_drq),
 * opt-in on the same handle and parameter arena.  serl_classifier_train_init replaces TrainState.create(tx=optax.adam(lr))
 * (reward_classifier.py:62-66): it allocates the Adam moments and the gradient of the trainable leaves (every camera head and the
 * classifier head; the trunk sits behind stop_gradient, resnet_v1.py:285-286, and its moments read as zeros) plus the
 * activations of max_batch rows.  Only optax.adam's b1 = 0.9, b2 = 0.999, eps = 1e-8 are accepted.  Every other training entry
 * point returns SERL_ERR_STATE on a handle without it, and SERL_ERR_INVALID for n > max_batch. */
int serl_classifier_train_init(serl_classifier* c, int max_batch, float lr, float b1, float b2, float eps);
/* One train_step (train_reward_classifier.py:122-137): dev_frames u8[n_cam][n][H][W][3] (device, already cropped),
 * dev_labels f32[n] (device); loss = mean(sigmoid_binary_cross_entropy(logits(train=True), labels)), accuracy from a
 * train=False forward of the same rows with the pre-update parameters, then one Adam step.  The two Dropout(0.1) layers use
 * dev_masks (device u8: [n_cam][n][4096] for encoder_def/encoder_<k>/Dropout_0, then [n][256] for the root Dropout_0) or,
 * when dev_masks is NULL, jax.random.bernoulli under host_mask_keys (host uint32[n_cam + 1][2]: the make_rng("dropout") keys
 * of those layers, cameras first), drawn inside the kernels that consume them. */
int serl_classifier_train_step(serl_classifier* c, const uint8_t* dev_frames, int n, const float* dev_labels,
                               const uint8_t* dev_masks, const uint32_t* host_mask_keys, void* stream);
/* apply_fn(..., train=True, rngs={"dropout": key}) (reward_classifier.py:20-28): train-mode logits, no update.  Same masks /
 * keys as serl_classifier_train_step; dev_logits f32[n] (device). */
int serl_classifier_train_forward(serl_classifier* c, const uint8_t* dev_frames, int n, const uint8_t* dev_masks,
                                  const uint32_t* host_mask_keys, float* dev_logits, void* stream);
/* (loss, train_accuracy) of the last step (train_reward_classifier.py:128,135); `out` device or host memory, copied on
 * `stream` */
int serl_classifier_read_train_info(serl_classifier* c, float out[2], void* stream);
/* TrainState.step / opt_state[0].count, and the Adam moments ("opt/mu", "opt/nu") of one leaf (frozen leaves: zeros) */
int serl_classifier_train_set_step(serl_classifier* c, int64_t step);
int serl_classifier_train_get_step(serl_classifier* c, int64_t* step_out);
int serl_classifier_train_set(serl_classifier* c, const char* section, const char* leaf, const float* host, int64_t count);
int serl_classifier_train_get(serl_classifier* c, const char* section, const char* leaf, float* host_out, int64_t count);

/* ---------------------------------------------------------------------------------------------
 * Behaviour cloning (agents/continuous/bc.py, built by utils/launcher.py:26-47 with encoder_type="resnet-pretrained").
 * One handle = BCAgent.state (params, one optax.adam(lr) state, step) + all activations; a separate handle so that
 * serl_agent_cfg and the DrQ path stay as they are.  Policy(EncodingWrapper(use_proprio, enable_stacking) over the frozen
 * trunk, MLP([256, 256], tanh, no LayerNorm, activate_final), heads mean / log_std, MultivariateNormalDiag (no tanh),
 * std = clip(exp(log_std), std_min, std_max) * sqrt(temperature)).
 * Leaves (flat fp32, HWIO kernels / [in][out] dense kernels): the trunk leaves of the agent ("trunk/..."),
 * "enc/<k>/{sle, dense/kernel, dense/bias, ln/scale, ln/bias}" (frozen: behind stop_gradient, encoding.py:48-49 and
 * actor_critic_nets.py:185), then the trainable "enc/proprio/{dense/kernel, dense/bias, ln/scale, ln/bias}",
 * "actor/{w1, b1, w2, b2}", "actor/mean/{kernel,bias}", "actor/logstd/{kernel,bias}".  Sections: "params", "opt/mu",
 * "opt/nu"; the moments of a frozen leaf read as zeros and may only be set to zeros.
 * --------------------------------------------------------------------------------------------- */
typedef struct serl_bc serl_bc;
typedef struct {
  int device, n_cam, H, W, state_dim, act_dim, max_batch;
  float lr;                 /* optax.adam learning rate (bc.py:134) */
  float dropout;            /* Dropout rate behind SpatialLearnedEmbeddings (resnet_v1.py:351) */
  float std_min, std_max;   /* launcher.py:41-42 */
} serl_bc_cfg;
int serl_bc_create(const serl_bc_cfg* cfg, serl_bc** out);   /* BCAgent.create (bc.py:118-204); the all-zero serl_bc_opts */
/* no_proprio 1: EncodingWrapper(use_proprio=False), BCAgent.create's own default (bc.py:126).  The code is the camera codes alone:
 * actor/w1 is (256 * n_cam, 256), there is no enc/proprio/... leaf or moment, the forward pass launches SpatialLearnedEmbeddings
 * without proprio rows, and the update has no proprio input-gradient GEMM, LayerNorm backward, column sum or weight-gradient
 * entry: the two MLP layers and the two heads alone train.  The state is never read: serl_batch.state and dev_state may be NULL
 * (state_dim is validated and matched as always).  Any value but 0 and 1 is SERL_ERR_INVALID. */
typedef struct serl_bc_opts {
  int no_proprio;
} serl_bc_opts;
int serl_bc_create_opts(const serl_bc_cfg* cfg, const serl_bc_opts* opts, serl_bc** out);
int serl_bc_use_proprio(serl_bc* c);   /* 1: proprio branch, 0: no_proprio, -1: NULL */
int serl_bc_destroy(serl_bc* c);
int serl_bc_num_leaves(serl_bc* c);
int serl_bc_leaf_info(serl_bc* c, int i, char* name_out, int name_cap, int64_t* count, int* trainable);
int serl_bc_set(serl_bc* c, const char* section, const char* leaf, const float* host, int64_t count);
int serl_bc_get(serl_bc* c, const char* section, const char* leaf, float* host_out, int64_t count);
int serl_bc_set_step(serl_bc* c, int64_t step);
int64_t serl_bc_get_step(serl_bc* c);
/* BCAgent.update (bc.py:37-77): frames[0] (the observations, [n_cam][batch][H][W][3]), state[0] and action of `batch`.
 * The Dropout keep-masks of the forward pass (train=True) are dev_masks u8[n_cam][batch][4096], or, when NULL, drawn inside
 * the SLE kernel as jax.random.bernoulli(key_c, 1 - dropout, (batch, 4096)) under host_mask_keys uint32[n_cam][2]. */
int serl_bc_update(serl_bc* c, const serl_batch* batch, const uint8_t* dev_masks, const uint32_t* host_mask_keys, void* stream);
/* info of the last update (bc.py:63-67): out[0] = actor_loss, out[1] = mse.  `out` is device or host memory; the copy is
 * ordered on `stream` (synchronise it before reading host memory) */
int serl_bc_read_info(serl_bc* c, float out[2], void* stream);
/* BCAgent.sample_actions (bc.py:79-97), train=False: argmax -> the mean (no tanh); otherwise mean + std * eps with
 * eps = dev_eps f32[n][A], or, when NULL, jax.random.normal(host_key, (n, A)).  dev_frames u8[n_cam][n][H][W][3],
 * dev_state f32[n][S], dev_actions_out f32[n][A]. */
int serl_bc_sample_actions(serl_bc* c, const uint8_t* dev_frames, const float* dev_state, int n, const float* dev_eps,
                           const uint32_t* host_key, float temperature, int argmax, float* dev_actions_out, void* stream);
/* BCAgent.get_debug_metrics (bc.py:99-116), train=False: per-sample mse[n], log_probs[n], pi_actions[n][A] (device) */
int serl_bc_debug_metrics(serl_bc* c, const serl_batch* batch, float* dev_mse, float* dev_logp, float* dev_pi, void* stream);

/* ---------------------------------------------------------------------------------------------
 * JAX's PRNG (threefry2x32, non-partitionable; jax/_src/prng.py, jax/_src/random.py of jax 0.4.x) -- csrc/jaxrng.hip.
 * The reference learner draws its crop offsets (vision/data_augmentations.py:7-36), REDQ indices (agents/continuous/sac.py:150-157),
 * policy noise (sac.py:118-132,197-201,224-227) and Dropout masks from jax.random and advances `state.rng` as
 * common/common.py:197-209, sac.py:287-289 and agents/continuous/drq.py:276-318 do.  These entry points reproduce that stream:
 * keys, integers and the 32-bit draws behind every sample are bit-exact; normals follow XLA's float32 erf_inv polynomial.
 * A key is uint32[2]; jax.random.PRNGKey(seed) = {0, seed & 0xffffffff} as the reference runs JAX (x64 disabled: the seed is an
 * int32, PRNGKey(-1) = {0, 0xffffffff}).  The host functions need no device.
 * --------------------------------------------------------------------------------------------- */
int serl_jax_prngkey(uint64_t seed, uint32_t key_out[2]);                              /* jax.random.PRNGKey */
int serl_jax_split(const uint32_t key[2], int num, uint32_t* keys_out /* [num][2] */); /* jax.random.split */
int serl_jax_fold_in(const uint32_t key[2], uint32_t data, uint32_t key_out[2]);       /* jax.random.fold_in */
int serl_jax_random_bits(const uint32_t key[2], int64_t n, uint32_t* out);             /* jax.random.bits(key, (n,)) */
int serl_jax_randint(const uint32_t key[2], int64_t n, int32_t minval, int32_t maxval, int32_t* out); /* jax.random.randint */
int serl_jax_normal_host(const uint32_t key[2], int64_t n, float* out);                /* jax.random.normal(key, (n,)) on the host */
/* batched_random_crop's offsets (data_augmentations.py:22-36): keys = split(key, frames); (y, x)_i = randint(keys[i], (2,), 0,
 * 2*padding + 1) -> yx_out int32[frames][2].  The SAME key serves every camera (drq.py:244-253). */
int serl_jax_crop_offsets(const uint32_t key[2], int frames, int padding, int32_t* yx_out);
/* Every key ONE learner call derives from state.rng, in the reference's order:
 *   drq_aug != 0 (DrQAgent.update_critics / update_high_utd, drq.py:276-277,307-308): rng, k_obs, k_next = split(rng, 3)
 *   then n_critic critic-only SACAgent.update calls and, if has_actor_temp, one actor + temperature update (sac.py:544-596); each:
 *     _, r_actor, r_critic, r_temp = split(rng, 4)                                          (common.py:197-200, sorted loss names)
 *     critic:  c, k_next_action = split(r_critic);  _, k_subsample = split(c)               (sac.py:137,151)
 *     actor:   _, k_policy, k_sample, _ = split(r_actor, 4);  _, k_temp = split(r_temp)     (sac.py:197,222)
 *     rng = split(rng)[0]                                                                   (sac.py:287-289)
 * k_next_action / k_policy / k_temp are BOTH the Dropout rng of that policy forward and (k_next_action, k_temp) its sample seed
 * (sac.py:122-128); k_sample seeds the policy-loss sample.  rng_out is state.rng after the call.
 * combined != 0 (SACAgent.update with all three networks, sac.py:243-299): ONE update whose critic, actor and temperature losses
 * take their keys from the same 4-way split (n_critic = 1, has_actor_temp = 1). */
#define SERL_JAX_MAX_UTD 32
typedef struct serl_jax_update_keys_t {
  uint32_t rng_out[2];
  uint32_t k_obs[2], k_next[2];
  int32_t n_critic;
  uint32_t k_next_action[SERL_JAX_MAX_UTD][2];
  uint32_t k_subsample[SERL_JAX_MAX_UTD][2];
  uint32_t k_policy[2], k_sample[2], k_temp[2];
} serl_jax_update_keys_t;
int serl_jax_update_keys(const uint32_t rng[2], int drq_aug, int n_critic, int has_actor_temp, int combined, serl_jax_update_keys_t* out);
/* serl_jax_update_keys, and the rngs the critic forwards of the same call run under (mlp.py:27-28 draws its Dropout masks from
 * them; sac.py:137-176,197-207):
 *   k_q_target[u]  c of `c, k_next_action = split(r_critic)`: forward_target_critic's rng                    (sac.py:137,143-147)
 *   k_q_online[u]  split(c)[0], what sac.py:151 leaves in `rng` for forward_critic (sac.py:174-176) -- or c itself with
 *                  subsample_none != 0 (critic_subsample_size None: no re-split, target and online forwards share rng and masks)
 *   k_q_actor      critic_rng, the fourth key of split(r_actor, 4)                                          (sac.py:197,203-207)
 * `keys` is filled exactly as serl_jax_update_keys fills it. */
typedef struct serl_jax_dropout_keys_t {
  uint32_t k_q_target[SERL_JAX_MAX_UTD][2];
  uint32_t k_q_online[SERL_JAX_MAX_UTD][2];
  uint32_t k_q_actor[2];
} serl_jax_dropout_keys_t;
int serl_jax_update_keys_dropout(const uint32_t rng[2], int drq_aug, int n_critic, int has_actor_temp, int combined, int subsample_none,
                                 serl_jax_update_keys_t* keys, serl_jax_dropout_keys_t* out);
/* Device draws: job i writes elements [first, first + count) of the flat array a JAX call of `n_total` elements returns
 * (a rank of a data-parallel job, or a minibatch window, fills its rows only):
 *   SERL_JAX_NORMAL       f32  jax.random.normal(key, shape)             SERL_JAX_BERNOULLI_U8  u8  jax.random.bernoulli(key, p, shape)
 *   SERL_JAX_BITS         u32  jax.random.bits(key, shape)
 * One launch for up to 16 jobs on `stream`. */
enum { SERL_JAX_NORMAL = 0, SERL_JAX_BERNOULLI_U8 = 1, SERL_JAX_BITS = 2 };
typedef struct serl_jax_job {
  uint32_t key[2];
  int32_t kind;
  float p;              /* bernoulli probability of a 1 */
  int64_t n_total, first, count;
  void* out;            /* device */
} serl_jax_job;
int serl_jax_fill(int device, const serl_jax_job* jobs, int n, void* stream);
/* Parameter initialisers (jax.nn.initializers.variance_scaling's draws, jax/_src/random.py of jax 0.4.x): job i writes the
 * whole flat f32 array of `count` elements that one call returns, times `scale` (float32 ops, in this order):
 *   SERL_JAX_INIT_UNIFORM           jax.random.uniform(key, shape, f32, minval, maxval) * scale
 *   SERL_JAX_INIT_TRUNCATED_NORMAL  jax.random.truncated_normal(key, minval, maxval, shape, f32) * scale
 *   SERL_JAX_INIT_NORMAL            jax.random.normal(key, shape, f32) * scale            (minval / maxval unused)
 * erf is XLA's float32 rational approximation, erf_inv XLA's ErfInv32 with log1p rounded from double precision, so that
 * device and host results agree bit for bit.  serl_jax_init_fill: one launch per 64 jobs on `stream`, `out` in device memory;
 * serl_jax_init_host: one job on the host, `out` in host memory. */
enum { SERL_JAX_INIT_UNIFORM = 0, SERL_JAX_INIT_TRUNCATED_NORMAL = 1, SERL_JAX_INIT_NORMAL = 2 };
typedef struct serl_jax_init_job {
  uint32_t key[2];
  int32_t kind;
  float minval, maxval;  /* uniform: [minval, maxval); truncated normal: the bounds (lower, upper) */
  float scale;
  int64_t count;
  void* out;
} serl_jax_init_job;
int serl_jax_init_fill(int device, const serl_jax_init_job* jobs, int n, void* stream);
int serl_jax_init_host(const serl_jax_init_job* job);

#ifdef __cplusplus
}
#endif
#endif /* SERL_MI355_H */
