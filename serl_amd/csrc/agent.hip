// DrQ / SAC agent: parameter arena, step orchestration and the agent half of the C ABI.
// Reference semantics (paths relative to serl_launcher/serl_launcher/):
//   agents/continuous/drq.py:255-328      update_high_utd / update_critics
//   agents/continuous/sac.py:118-299      losses, update(); :544-596 update_high_utd
//   common/common.py:124-221              3 Adam txs over the full tree, summed updates, target EMA
//   common/encoding.py:26-72              per-camera encode + proprio branch
// The frozen trunk is evaluated twice per update (augmented obs, augmented next_obs); the reference
// evaluates it a third time with target_params, whose trunk leaves equal the online ones up to
// EMA round-off (<= 1e-6 relative) -- the target copy is still maintained for export.
// LIVE TRUNK (serl_mi355.h at serl_agent_create): with adamw on an agent that has the pretrained trunk the optimizers decay the
// trunk at every step, the two copies differ, and that third evaluation is real: live_features below.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dense_layer.h"
#include "small_encoder.h"

using namespace serl;

namespace {

constexpr int kL = SERL_MAX_MLP_LAYERS;
// K-split depth of an MLP layer's forward GEMM: the layer on the network's input is the deepest (it has the longest K)
inline int critic_smax(int layer) { return layer == 0 ? 4 : 2; }
inline int policy_smax(int layer) { return layer == 0 ? 8 : 4; }

struct Offs {
  long enc0, cam_stride;   // camera 0's first leaf (SpatialLearnedEmbeddings kernel, or the SmallEncoder's first conv); camera k's sit k * cam_stride further
  DenseLn cam, prop;       // the Dense -> LayerNorm -> activation layers: camera bottleneck, proprio branch,
  DenseLn c[kL], a[kL];    // ... and the nc layers of the critic's MLP, the na layers of the policy's (mlp.py:19-31), input side first
  int nc, na;
  long c_hw, c_hb;
  long a_Wm, a_bm, a_Ws, a_bs;   // kPolUniform: a_bs = actor/log_stds, no a_Ws; kPolFixed: neither (both -1)
  long lam;
  long P, Pc, Pa0, Pa1;
};

struct EncBuf {     // activations of one EncodingWrapper forward
  float* f;         // [n_cam][B][D] SLE output (after dropout)
  float* xhat;      // [n_cam*B][bottleneck]
  float* rstd;      // [n_cam*B]
  float* pxhat;     // [B][proprio_dim]
  float* prstd;     // [B]
  float* enc;       // [B][ld] output slice base
  long ld;
};
struct LayerBuf { float *h, *xhat, *rstd; };   // a layer's output [rows][width], normalised pre-activation and 1/std [rows]
struct MlpBuf { LayerBuf l[kL]; };              // an MLP's activations, one LayerBuf per layer of that layer's width (ensemble: rows = E*B)
struct GradBuf { float *dy, *dpre, *dg; };      // a layer's backward scratch: DenseLnGrad's three tensors
struct CritBuf {
  float* x;  // [B][E+A]
  MlpBuf m;
  float* q;  // [ens][B]
};
struct PolBuf {
  MlpBuf m;
  float *pre, *std, *logp;  // [2][B][A], [B][A], [B]
};

constexpr int kScalars = 32;
// scalar slots (device): local sums that are all-reduced together with the gradients
enum { S_D2 = 0, S_Q = 1, S_Y = 2, S_QPI = 3, S_LOGP = 4, S_LOGP_NEXT = 5 };
// aux slots (device, rank-local, never all-reduced)
enum { X_ALPHA = 0, X_TGRAD = 1, X_NORM2 = 2 /* [2] */, X_N = 8 };
// info accumulator slots
enum { I_CL = 0, I_PQ, I_TQ, I_AL, I_TEMP, I_ENT, I_TL, I_N };
// adam_ema_kernel's info rider (heads.hip) indexes these slots by number
static_assert(S_D2 == 0 && S_Q == 1 && S_Y == 2 && S_QPI == 3 && S_LOGP == 4 && S_LOGP_NEXT == 5, "scalar slots");
static_assert(I_CL == 0 && I_PQ == 1 && I_TQ == 2 && I_AL == 3 && I_TEMP == 4 && I_ENT == 5 && I_TL == 6 && I_N <= 8, "info slots");

}  // namespace

struct serl_agent {
  serl_agent_cfg cfg{};
  int E = 0, D = 0, HW = 0, XA = 0;  // enc dim, sle dim, feature pixels, E + A
  bool state_only = false;           // n_cam == 0: SACAgent.create_states
  bool small = false;                // encoder_type == "small": trainable SmallEncoder instead of the frozen trunk
  bool prop = false;                 // the EncodingWrapper has its proprio branch (cameras and opts.no_proprio == 0); else nothing reads cur.state
  // The network options the agent was created with (serl_mi355.h, NETWORK OPTIONS), normalised by create_agent: both networks have
  // n_layers >= 1 and their dims filled ({cfg.hidden, cfg.hidden} where 0 layers were given: nothing below reads cfg.hidden), and
  // fixed_std points into the vector below.  act is a kAct* code; no_layer_norm is read by build_layout alone, the layers carry it
  // from there (DenseLn::ln).
  serl_agent_opts opts{};
  // opts.ragged_widths: the dims above are the STORAGE widths, 64 ceil(d / 64), and everything that launches reads them as it
  // always did; the widths the agent was created with are true_dims[network][layer] (equal to the dims without the option).  A
  // layer off the grid keeps its leaves as boxes in zero padding (param_arena.h) and its LayerNorm rows divide by the true width.
  int true_dims[2][SERL_MAX_MLP_LAYERS] = {};
  int pol_mode = kPolExp;            // opts.std_param / no_tanh as the head kernels take them
  int head_groups = 2;               // Dense layers of the policy head: (mean, log_std), or the mean alone with kPolUniform / kPolFixed
  // SERL_STD_FIXED: the constant std vector of a kPolFixed agent as it was passed, [act_dim]; the device copy is an
  // allocation of its own outside the arena (no leaf, no moments, no target copy, never all-reduced).  Empty / nullptr otherwise.
  std::vector<float> fixed_std;
  float* fixed_std_dev = nullptr;
  // mlp_bound: what serl_agent_set_mlp_noise left for the next update / phase / dry-run call; mlp_cur: what the call in progress
  // (mlp_depth > 0: its outermost entry point took the binding) reads.  MlpNoiseScope, below.
  serl_mlp_noise mlp_bound{}, mlp_cur{};
  int mlp_depth = 0;
  SmallWorkspace sws{};
  Offs o{};
  std::vector<Leaf> theta_leaves, trunk_leaves;
  long trunk_count = 0;
  TrunkOffsets to{};
  // device memory
  void* arena = nullptr;
  float *trunk = nullptr, *trunk_t = nullptr, *theta = nullptr, *theta_t = nullptr;
  float *m_c = nullptr, *v_c = nullptr, *m_a = nullptr, *v_a = nullptr, *m_t = nullptr, *v_t = nullptr;
  float* G = nullptr;  // [Gc (Pc) | scalars (32) | Ga (Pa1-Pa0)]
  float *Gc = nullptr, *SC = nullptr, *Ga = nullptr;
  float* info_acc = nullptr;  // [I_N]
  float* eval_info = nullptr; // [I_N] the same scalars as serl_agent_eval_losses forms them: an update's info is never overwritten
  float* aux = nullptr;       // [X_N]
  TrunkWeights tw{};
  TrunkWorkspace tws{};
  TrunkPacked tpk{};
  int trunk_mode = 1;  // 0: exact fp32 MFMA convs, 1: split-fp16 (f16x3) convs for the blocks
  // Live trunk: the pretrained trunk under adamw.  The target copy has its own weights view and packed planes (re-derived by
  // trunk_forward when an apply marked them dirty), and every slot a buffer [n_cam][batch] of next-frame features of the target
  // trunk.  trunk_ver / trunk_t_ver count the changes of either copy; feats_on / feats_tg say which rows of the selected batch
  // hold features of which version (live_features computes what a phase lacks).  All of it unused, and nothing allocated, otherwise.
  bool live = false;
  TrunkWeights tw_t{};
  TrunkPacked tpk_t{};
  float* feats_t = nullptr;   // current slot
  float* feats_t_slot[4] = {nullptr, nullptr, nullptr, nullptr};
  int64_t trunk_ver = 0, trunk_t_ver = 0;
  struct FeatRows { int64_t ver = -1; int lo = 0, hi = 0; } feats_on, feats_tg;
  // last-arriver fusion of the update chain (heads.hip): slab reductions / the tanh-Gaussian head run inside the GEMM
  // launches that feed them, the critic loss rides on the LayerNorm backward that consumes dQ, noise is hashed where it is used.
  // SERL_CHAIN_FUSE=0 restores one launch per operation (A/B timing; the fused path is bit-identical on identical noise).
  bool fuse = true;
  // K-split budget of the chain's GEMMs (workgroups per launch): 512 by default; 256 when the caller overlaps the chain with the
  // next batch's trunk pass at a large per-rank batch (serl_agent_set_chain_budget) -- fewer workgroups queue for CU slots
  // between conv workgroups (same call: pipelined 2.605 -> 2.570 ms, conv_init next to the chain 455 -> 372 us; alone the
  // chain is 2 % slower with it, and 1024 - 2048 would be 3 - 4 % faster alone)
  long split_budget = 0;
  int* ctr = nullptr;   // arrival counters: kCtrLanes ranges of kCtrPerLane (zero between launches)
  float* feats = nullptr;  // current slot: [2][n_cam][B][HW][512]
  static constexpr int kSlots = 3;                                  // pipelined update batches in flight (see serl_mi355.h)
  float* feats_slot[kSlots + 1] = {nullptr, nullptr, nullptr, nullptr};   // 0..kSlots-1: update batches, kSlots: sample_actions and the read-only evaluations
  serl_batch cur_slot[kSlots]{};
  bool slot_valid[kSlots] = {false, false, false};
  EncBuf encP{}, encT{}, encO{};
  CritBuf critT{}, crit{};
  PolBuf pol{}, polT{};
  float* slabs = nullptr; long slabs_cap = 0;  // GEMM split-K scratch (== slabs_lane[0])
  float* slabs_lane[3] = {nullptr, nullptr, nullptr};  // one per instance of a multi-instance launch
  float *dq = nullptr, *ytgt = nullptr;
  // MLP layer j (critic and policy in turn; the deferred gradient jobs of a phase read dpre / dg at its end: no two layers share),
  // camera bottleneck (dy lies in dx), proprio branch
  GradBuf s[kL]{}, scam{}, sprop{};
  float *dx = nullptr, *df = nullptr, *sle_part = nullptr, *dpre = nullptr;
  float *eps_buf[3] = {nullptr, nullptr, nullptr};
  uint8_t* mask_buf[3] = {nullptr, nullptr, nullptr};
  float* act_tmp = nullptr;  // [B][A] sample_actions scratch
  // batch of the current update (caller-owned device memory)
  serl_batch cur{};
  bool has_batch = false;
  // The target copy of the FROZEN trunk takes an EMA step per critic update like every other leaf (common.py:124-134), but no
  // gradient or weight decay ever reaches those leaves (with adamw the trunk is `live` and never takes this path), so the steps are only counted here
  // and applied in one pass (frozen_ema: the same rounding sequence) when somebody reads or overwrites the trunk's target
  // leaves -- 59 MB less HBM traffic per critic step.
  int64_t trunk_ema_pending = 0;
  // optimizer bookkeeping
  int64_t step = 0;
  uint64_t noise_ctr = 0;
  serl_info last_info{};
  float lr_last[3] = {0.f, 0.f, 0.f};   // learning rates of the last apply, indexed by SERL_TX_*
  int last_global = 0;
  bool info_reset = true;
  // batch-sharded data parallelism: this rank's local batch is rows [shard_off, shard_off + local) of a global
  // batch of shard_global rows (0 = not sharded); device noise is indexed by the global row
  int64_t shard_off = 0, shard_global = 0;
  // the parameter-gradient kernels of a phase -- nothing downstream of the input-gradient chain needs them before
  // the optimizer -- are queued and issued as ONE column-sum launch and ONE grouped weight-gradient GEMM at the end
  // of the phase (flush_param_grads): 8 fewer dependent kernel boundaries per grad-step pair
  bool pg_defer = false;
  Colsum3Args pg_cs[kMaxColsum];
  int pg_ncs = 0;
  GemmDesc pg_wg[kMaxGemmGroups];
  int pg_nwg = 0;
  // Reward labelling (vice.py:546,594): with a reward classifier attached, update_critics / update_high_utd replace the batch's
  // rewards by (sigmoid(classifier(augmented next_obs, train=False)) >= 0.5), computed once per call into `labels`; the critic
  // loss then reads `labels` instead of cur.reward (`labelled`, cleared when another batch is selected).  label_mode
  // SERL_LABEL_FEATURES: the classifier's head runs on the slot's pass-1 trunk features (the trunks were bit-identical at
  // attach); SERL_LABEL_FRAMES: the classifier's own trunk runs on the batch's next frames.  The handle is borrowed.
  serl_classifier* cls = nullptr;
  int cls_cam[SERL_MAX_CAMS] = {0, 0, 0, 0};   // classifier camera k reads agent camera cls_cam[k]
  int label_mode = SERL_LABEL_NONE;
  int64_t trunk_gen = 0;                       // bumped by every trunk leaf set on this agent
  int64_t attach_gen = 0, attach_cls_gen = 0;  // both generations when the classifier was attached
  float *labels = nullptr, *label_logits = nullptr, *label_mean = nullptr;   // [batch], [batch], [1]
  int* label_ctr = nullptr;
  int label_n = 0;                             // rows of the last labelling
  bool labelled = false, label_exempt = false; // exempt: SACAgent.update, which VICE does not override
  int snapshots = 0;                           // live serl_snapshot handles (snapshot.hip): serl_agent_destroy is refused while > 0
};

namespace {

constexpr int kSleSplit = 8;
constexpr int kCtrPerLane = 4096, kCtrLanes = kMaxGemmGroups;
long pad64(long x) { return (x + 63) / 64 * 64; }
// the parameter-gradient kernels of a phase are always deferred to the end of the phase (issuing them layer by layer was
// measured 3 % slower at a per-rank batch of 32, equal at 256)

void build_layout(serl_agent* a) {
  const serl_agent_cfg& c = a->cfg;
  const TrunkDims d = c.n_cam > 0 ? trunk_dims(c.H, c.W) : TrunkDims{};
  a->state_only = c.n_cam == 0;
  a->small = !a->state_only && c.encoder_type == SERL_ENCODER_SMALL;
  a->HW = (a->state_only || a->small) ? 0 : d.h[5] * d.w[5];
  a->D = a->state_only ? 0 : (a->small ? kSmallFeat[kSmallLayers] : 512 * c.sle_features);
  a->prop = !a->state_only && !a->opts.no_proprio;
  a->E = a->state_only ? c.state_dim : c.bottleneck * c.n_cam + (a->prop ? c.proprio_dim : 0);
  a->XA = a->E + c.act_dim;
  long off = 0;
  Offs& o = a->o;
  std::vector<Leaf>& L = a->theta_leaves;
  const int N = c.ensemble;
  const long A = c.act_dim;
  const serl_mlp_opts &critic = a->opts.critic, &policy = a->opts.policy;
  const int Hc = critic.dims[critic.n_layers - 1], Hp = policy.dims[policy.n_layers - 1];   // the widths the heads read
  const int Hct = a->true_dims[0][critic.n_layers - 1], Hpt = a->true_dims[1][policy.n_layers - 1];   // ... and their live rows
  const auto mlp_leaves = [&](DenseLn* layers, const std::string& name, const serl_mlp_opts& net, int groups, int in) {
    const int* td = a->true_dims[&net == &policy];
    for (int j = 0; j < net.n_layers; ++j) {
      const std::string k = std::to_string(j + 1);
      layers[j] = add_dense_ln_leaves(L, off, name + "/w" + k, name + "/b" + k, name + "/ln" + k, groups, j ? net.dims[j - 1] : in, net.dims[j],
                                      net.act, net.dropout, !net.no_layer_norm, j ? td[j - 1] : in, td[j]);
    }
  };
  const CamHeadOffsets ch = add_cam_head_leaves(L, off, c.n_cam, a->D, c.bottleneck, [&](const std::string& p) {
    if (!a->small) { add_leaf(L, off, p + "sle", (long)a->HW * 512 * c.sle_features); return; }
    for (int l = 0; l < kSmallLayers; ++l) {   // per layer [9*cin + 1][cout]: kernel (HWIO) immediately followed by the bias (small_encoder.hip)
      // (layer 0 of a stacked agent takes the T frames as 3T channels: kernel (3,3,3T,32), common/encoding.py:39-44)
      add_leaf(L, off, p + "conv" + std::to_string(l) + "/kernel", 9L * kSmallFeat[l] * (l == 0 ? c.num_stack : 1) * kSmallFeat[l + 1]);
      add_leaf(L, off, p + "conv" + std::to_string(l) + "/bias", kSmallFeat[l + 1]);
    }
  });
  o.enc0 = ch.first; o.cam_stride = ch.stride; o.cam = ch.dense;
  o.nc = critic.n_layers; o.na = policy.n_layers;
  mlp_leaves(o.c, "critic", critic, N, a->XA);
  // DrQ: one Dense(1) head shared by the ensemble (drq.py:201-207); state-only SAC: ensemblize vmaps the whole
  // Critic, so every member has its own head (actor_critic_nets.py:49-73,156-164)
  // (the heads read the last layer's storage width: the rows of their kernels behind the true width are zero padding)
  o.c_hw = add_leaf_box(L, off, "critic/head/kernel", a->state_only ? N : 1, 1, Hct, 1, Hc);
  o.c_hb = add_leaf(L, off, "critic/head/bias", a->state_only ? N : 1);
  o.Pa0 = off;
  if (a->prop) {
    o.prop = add_dense_ln_leaves(L, off, "enc/proprio/dense/kernel", "enc/proprio/dense/bias", "enc/proprio/ln", 1, c.state_dim,
                                 c.proprio_dim, kActTanh);
  }
  o.Pc = off;
  mlp_leaves(o.a, "actor", policy, 1, a->E);
  o.a_Wm = add_leaf_box(L, off, "actor/mean/kernel", 1, Hpt, A, Hp, A);
  o.a_bm = add_leaf(L, off, "actor/mean/bias", A);
  const int std_param = a->opts.std_param;
  a->pol_mode = std_param | (a->opts.no_tanh ? kPolNoTanh : 0);
  a->head_groups = (std_param == SERL_STD_UNIFORM || std_param == SERL_STD_FIXED) ? 1 : 2;
  if (std_param == SERL_STD_FIXED) {   // no std parameter at all (actor_critic_nets.py:190-192): the head ends with the mean's bias
    o.a_Ws = o.a_bs = -1;
  } else if (a->head_groups == 1) {   // one log-std vector shared by all rows (actor_critic_nets.py:199-201), directly behind the mean's bias
    o.a_Ws = -1;
    o.a_bs = add_leaf(L, off, "actor/log_stds", A);
  } else {
    o.a_Ws = add_leaf_box(L, off, "actor/logstd/kernel", 1, Hpt, A, Hp, A);
    o.a_bs = add_leaf(L, off, "actor/logstd/bias", A);
  }
  o.Pa1 = off;
  o.lam = add_leaf(L, off, "temp/lagrange", 1);
  o.P = off;
  // trunk
  off = 0;
  a->trunk_count = 0;
  if (a->state_only || a->small) return;   // no frozen trunk
  a->to = add_trunk_leaves(a->trunk_leaves, off);
  a->trunk_count = off;
}

// carve everything (pass 1 with base == nullptr measures)
size_t carve(serl_agent* a, void* base) {
  const serl_agent_cfg& c = a->cfg;
  const long B = c.batch, N = c.ensemble, A = c.act_dim;
  const Offs& o = a->o;
  // the widest layer of either MLP (shared scratch is sized by it) and the critic's last (the head gradient's width)
  const serl_mlp_opts &critic = a->opts.critic, &policy = a->opts.policy;
  const long Wc = *std::max_element(critic.dims, critic.dims + critic.n_layers);
  const long Wp = *std::max_element(policy.dims, policy.dims + policy.n_layers);
  const long Hc = critic.dims[critic.n_layers - 1];
  Bump b(base);
  a->trunk = b.take<float>(a->trunk_count);
  a->trunk_t = b.take<float>(a->trunk_count);
  a->theta = b.take<float>(o.P);
  a->theta_t = b.take<float>(o.P);
  a->m_c = b.take<float>(o.Pc); a->v_c = b.take<float>(o.Pc);
  a->m_a = b.take<float>(o.Pa1 - o.Pa0); a->v_a = b.take<float>(o.Pa1 - o.Pa0);
  a->m_t = b.take<float>(1); a->v_t = b.take<float>(1);
  a->G = b.take<float>(o.Pc + kScalars + (o.Pa1 - o.Pa0));
  a->Gc = a->G; a->SC = a->G ? a->G + o.Pc : nullptr; a->Ga = a->G ? a->G + o.Pc + kScalars : nullptr;
  a->info_acc = b.take<float>(8);
  a->aux = b.take<float>(X_N);
  const size_t persistent = b.off;  // zero-initialised region ends here
  // (the scratch slot holds both observation sides too: serl_agent_eval_losses runs a whole batch through it)
  for (int k = 0; k <= serl_agent::kSlots; ++k)
    a->feats_slot[k] = b.take<float>(2L * c.n_cam * B * a->HW * 512);   // (HW = 0 without a trunk)
  a->feats = a->feats_slot[0];
  auto enc = [&](EncBuf& e) {
    e.f = b.take<float>((long)c.n_cam * B * a->D);
    e.xhat = b.take<float>((long)c.n_cam * B * c.bottleneck);
    e.rstd = b.take<float>((long)c.n_cam * B);
    e.pxhat = a->opts.no_proprio ? nullptr : b.take<float>(B * c.proprio_dim);   // (no proprio scratch without the branch)
    e.prstd = a->opts.no_proprio ? nullptr : b.take<float>(B);
    e.enc = nullptr; e.ld = 0;
  };
  enc(a->encP); enc(a->encT); enc(a->encO);
  float* encP_out = b.take<float>(B * a->E);
  a->encP.enc = encP_out; a->encP.ld = a->E;
  auto mlp = [&](MlpBuf& m, long rows, const serl_mlp_opts& net) {
    for (int j = 0; j < net.n_layers; ++j) {
      LayerBuf* l = &m.l[j];
      l->h = b.take<float>(rows * net.dims[j]); l->xhat = b.take<float>(rows * net.dims[j]); l->rstd = b.take<float>(rows);
    }
  };
  auto crit = [&](CritBuf& cb) {
    cb.x = b.take<float>(B * a->XA);
    mlp(cb.m, N * B, critic);
    cb.q = b.take<float>(N * B);
  };
  crit(a->critT); crit(a->crit);
  a->encT.enc = a->critT.x; a->encT.ld = a->XA;
  a->encO.enc = a->crit.x; a->encO.ld = a->XA;
  for (PolBuf* pbuf : {&a->pol, &a->polT}) {
    mlp(pbuf->m, B, policy);
    pbuf->pre = b.take<float>(2 * B * A); pbuf->std = b.take<float>(B * A); pbuf->logp = b.take<float>(B);
  }
  // (fused epilogues keep whole 64x64 slab tiles: rows and columns padded to 64).  The terms, in order: the camera heads' K-split
  // (32 slices), the critic's input gradient summed over members, a policy layer (K-split <= 8), a critic layer (K-split <= 4 per
  // member) and the shared head's gradient (K-split 8, 64 padded rows); every user checks its own need against slabs_cap with the
  // numbers in the message (hidden = 1024 x 16 members x 65 rows: tests/test_mlp_widths_gpu.py).  The lanes are shared by all
  // layers: the policy's and the critic's terms take the widest layer of their MLP, the head gradient the critic's last width.
  const long Bp = pad64(B);
  long cap = std::max<long>({(long)c.n_cam * 32 * Bp * c.bottleneck, N * Bp * pad64(a->XA), 8 * Bp * Wp, 4 * N * Bp * Wc, 16L * 64 * Hc});
  a->slabs_cap = cap;
  for (int k = 0; k < 3; ++k) a->slabs_lane[k] = b.take<float>(cap);
  a->slabs = a->slabs_lane[0];
  a->dq = b.take<float>(N * B); a->ytgt = b.take<float>(B);
  for (int j = std::max(critic.n_layers, policy.n_layers) - 1; j >= 0; --j) {   // layer j's scratch holds the critic's layer j or the policy's, whichever is larger
    const long n = std::max<long>(j < critic.n_layers ? N * B * critic.dims[j] : 0, j < policy.n_layers ? B * policy.dims[j] : 0);
    GradBuf* s = &a->s[j];
    s->dy = b.take<float>(n); s->dpre = b.take<float>(n); s->dg = b.take<float>(n);
  }
  a->dx = b.take<float>(B * a->XA);
  a->scam.dpre = b.take<float>((long)c.n_cam * B * c.bottleneck);
  a->scam.dg = b.take<float>((long)c.n_cam * B * c.bottleneck);
  a->df = b.take<float>((long)c.n_cam * B * a->D);
  a->sle_part = b.take<float>((long)c.n_cam * kSleSplit * a->HW * 512 * c.sle_features);
  const long Bprop = a->opts.no_proprio ? 0 : B * c.proprio_dim;
  a->sprop.dpre = b.take<float>(Bprop); a->sprop.dg = b.take<float>(Bprop);
  a->dpre = b.take<float>(2 * B * A); a->sprop.dy = b.take<float>(Bprop);
  for (int k = 0; k < 3; ++k) {
    a->eps_buf[k] = b.take<float>(B * A);
    a->mask_buf[k] = b.take<uint8_t>((long)c.n_cam * B * a->D);
  }
  a->act_tmp = b.take<float>(B * A);
  a->ctr = b.take<int>((long)kCtrPerLane * kCtrLanes);
  a->labels = b.take<float>(B); a->label_logits = b.take<float>(B); a->label_mean = b.take<float>(1);
  a->label_ctr = b.take<int>(1);
  a->eval_info = b.take<float>(8);
  if (a->small) {
    void* smem = b.take<uint8_t>(small_workspace_bytes(c.n_cam * c.batch, c.H, c.W, c.num_stack));
    if (base) small_workspace_bind(a->sws, smem, c.n_cam * c.batch, c.H, c.W, c.num_stack);
  } else if (!a->state_only) {
    const int nimg = 2 * c.n_cam * c.batch;
    void* tmem = b.take<uint8_t>(trunk_workspace_bytes(nimg, c.H, c.W));
    if (base) trunk_workspace_bind(a->tws, tmem, nimg, c.H, c.W);
    void* pmem = b.take<uint8_t>(trunk_packed_bytes());
    if (base) trunk_packed_bind(a->tpk, pmem);
    if (a->live) {   // the target copy's planes and, per slot, its features of the next frames
      static_assert(sizeof(a->feats_t_slot) / sizeof(a->feats_t_slot[0]) == serl_agent::kSlots + 1, "one target-feature buffer per slot");
      void* pmem_t = b.take<uint8_t>(trunk_packed_bytes());
      if (base) trunk_packed_bind(a->tpk_t, pmem_t);
      for (int k = 0; k <= serl_agent::kSlots; ++k) a->feats_t_slot[k] = b.take<float>((long)c.n_cam * B * a->HW * 512);
      a->feats_t = a->feats_t_slot[0];
    }
  }
  (void)persistent;
  return b.off;
}

// K-split of a GEMM launch: as deep as `smax` for latency when the problem is small, but never more
// workgroups than the budget -- at large per-rank batches the update chain runs beside the trunk of the
// next batch and every extra workgroup waits for a conv workgroup to retire.
// `agent_budget` is the calling agent's own serl_agent_set_chain_budget value (0 = default): no process-global state, so two
// agents (or sample_actions on another thread) never see each other's budget.
int split_for(long agent_budget, int M, int N, int groups, int smax, long budget = 0) {
  if (budget <= 0) budget = agent_budget > 0 ? agent_budget : 512L;
  return split_under(M, N, groups, smax, budget);
}

// ---- EncodingWrapper forward on precomputed trunk features (encoding.py:26-72) ------------------
// Up to kMaxMulti independent instances (parameter vector x observation side x dropout mask) in four
// launches: SpatialLearnedEmbeddings, bottleneck Dense (K-split GEMM), LayerNorm+tanh, proprio branch.
// Instance i uses split-K scratch slabs_lane[i].  Samples [off, off+cnt) of the current batch.
struct EncJob {
  const float* P;        // parameter vector (online or target)
  int which;             // 0 = observations, 1 = next_observations
  const uint8_t* mask;   // dropout keep-mask, nullptr = train=False
  EncBuf* e;
  const float* act_src;  // optional rider: copy [cnt][A] actions (ld A) to act_dst (ld XA)
  float* act_dst;
  int gen_mask = 0;            // fused chain, mask == nullptr: 1 = hash the Dropout keep-mask inside the SLE kernel from mask_seed,
  uint64_t mask_seed = 0;      // 2 = jax.random.bernoulli(tf_key[camera], keep, (tf_rows, D)) rows tf_row0.. (serl_noise key_mask_*)
  const uint32_t* tf_key = nullptr; long tf_rows = 0, tf_row0 = 0;
  const float* x = nullptr;    // trunk features [n_cam][cfg.batch] to read instead of side `which` of the slot (live trunk: the target copy's)
};
// The tensors of the two encoder layers in one EncodingWrapper pass: every camera reads its own block of f and writes its
// columns of the code; the proprio branch reads `state` and writes the columns behind the cameras'.
DenseLnIo cam_io(const serl_agent* a, const EncBuf& e) {
  return DenseLnIo{e.f, a->D, (long)a->cfg.batch * a->D, e.enc, e.ld, a->cfg.bottleneck, e.xhat, e.rstd};
}
DenseLnIo prop_io(const serl_agent* a, const EncBuf& e, const float* state) {
  return DenseLnIo{state, a->cfg.state_dim, 0, e.enc + (long)a->cfg.n_cam * a->cfg.bottleneck, e.ld, 0, e.pxhat, e.prstd};
}
int encode_multi(serl_agent* a, const EncJob* jobs, int n, int off, int cnt, hipStream_t st) {
  const serl_agent_cfg& c = a->cfg;
  const Offs& o = a->o;
  const long Bfull = a->cur.batch;
  SERL_REQUIRE(n >= 1 && n <= 3, "bad encode instance count");
  if (a->state_only) {  // encoder=None: the "encoding" is the state vector itself (+ the actions rider)
    CopyJob cj[kMaxMulti];
    int m = 0;
    for (int i = 0; i < n; ++i) {
      const EncJob& j = jobs[i];
      cj[m++] = CopyJob{a->cur.state + ((long)j.which * Bfull + off) * c.state_dim, c.state_dim, j.e->enc, j.e->ld, c.state_dim};
      if (j.act_dst) cj[m++] = CopyJob{j.act_src, c.act_dim, j.act_dst, a->XA, c.act_dim};
    }
    return copy_cols_multi(cj, m, cnt, st);
  }
  SleFwdArgs sv[3];
  GemmDesc gd[3];
  LnFwdArgs lv[3];
  ProprioArgs pv[3];
  bool any_rider = false;   // image-only agents: some instance carries the actions rider
  const int S = split_for(a->split_budget, cnt, c.bottleneck, c.n_cam * n, 32);  // K = 4096: up to 32 slices of 128
  for (int i = 0; i < n; ++i) {
    const EncJob& j = jobs[i];
    EncBuf& e = *j.e;
    sv[i] = SleFwdArgs{};
    sv[i].x = (j.x ? j.x : a->feats + ((long)j.which * c.n_cam) * c.batch * a->HW * 512) + (long)off * a->HW * 512;
    sv[i].K = j.P + o.enc0;
    sv[i].mask = j.mask ? j.mask + (long)off * a->D : nullptr;
    sv[i].f = e.f;
    gd[i] = layer_fwd(o.cam, j.P, cam_io(a, e), cnt, a->slabs_lane[i], S);
    lv[i] = layer_ln_fwd(o.cam, j.P, cam_io(a, e), cnt, gd[i]);
    ProprioArgs& pr = pv[i];
    pr = ProprioArgs{};   // (without the proprio branch: the rider's fields alone, and the state is not touched)
    if (a->prop) pr = layer_row_fwd(o.prop, j.P, prop_io(a, e, a->cur.state + ((long)j.which * Bfull + off) * c.state_dim));
    else any_rider = any_rider || j.act_dst;
    if (j.act_dst) {
      pr.copy_src = j.act_src; pr.ld_copy_src = c.act_dim; pr.copy_dst = j.act_dst; pr.ld_copy_dst = a->XA;
      pr.copy_cols = c.act_dim;
    }
  }
  if (a->fuse) {
    for (int i = 0; i < n; ++i) {
      sv[i].gen = jobs[i].gen_mask; sv[i].seed = jobs[i].mask_seed;
      sv[i].row_offset = a->shard_off + off; sv[i].rows_global = a->shard_global ? a->shard_global : Bfull;
      if (jobs[i].gen_mask == 2) sle_tf_masks(sv[i], jobs[i].tf_key, c.n_cam, jobs[i].tf_rows, jobs[i].tf_row0);
    }
  }
  if (a->small) {   // trainable conv stack + average pool per (parameter vector, observation side); no dropout (pool "avg")
    const size_t fbytes = (size_t)c.H * c.W * 3;
    // (no Dropout on this encoder -- pool "avg" -- so two instances with the same parameters and observation side are the same
    //  pass: the actor step's critic-side and policy-side encodings of obs.  The LAST instance always runs: the backward pass
    //  reads the activations of the forward pass that ran last.)
    for (int i = 0; i < n; ++i) {
      const EncJob& j = jobs[i];
      int dup = -1;
      for (int k = i + 1; k < n; ++k)
        if (jobs[k].P == j.P && jobs[k].which == j.which) dup = k;
      if (dup >= 0) { gd[i].A = jobs[dup].e->f; continue; }
      const uint8_t* fr = a->cur.frames + (((size_t)j.which * c.n_cam) * Bfull + off) * c.num_stack * fbytes;   // an image = T frames
      RC(small_forward(a->sws, j.P, o.enc0, o.cam_stride, fr, Bfull, c.n_cam, cnt, j.e->f, (long)c.batch * a->D, st));
    }
  } else if (a->fuse) {   // channel-blocked SLE (+ hashed Dropout mask) with the proprio branch as extra workgroups of the launch
    // (an image-only agent: no proprio rows; the rider's rows alone behind the SLE workgroups, and none without a rider)
    RC(sle_proprio_fwd_multi(sv, a->prop || any_rider ? pv : nullptr, n, 1.0f - c.dropout, cnt, a->HW, 512, c.n_cam, (long)c.batch * a->HW * 512, o.cam_stride,
                             Bfull * a->D, (long)c.batch * a->D, c.state_dim, st));
  } else {
    RC(sle_fwd_multi(sv, n, 1.0f / (1.0f - c.dropout), cnt, a->HW, 512, c.n_cam, (long)c.batch * a->HW * 512, o.cam_stride,
                     Bfull * a->D, (long)c.batch * a->D, st));
  }
  RC(gemm_f32_multi(gd, n, st));
  RC(ln_fwd_multi(lv, n, c.bottleneck, st));
  if (a->fuse && !a->small) return SERL_OK;   // (the proprio branch rode on the SLE launch)
  if (a->prop) return proprio_fwd_multi(pv, n, c.state_dim, cnt, st);
  // image-only: where the proprio rows are a launch of their own, the rider is a column copy in its place (none without a rider)
  CopyJob cj[kMaxMulti];
  int m = 0;
  for (int i = 0; i < n; ++i)
    if (jobs[i].act_dst) cj[m++] = CopyJob{jobs[i].act_src, c.act_dim, jobs[i].act_dst, a->XA, c.act_dim};
  return m ? copy_cols_multi(cj, m, cnt, st) : SERL_OK;
}

// The tensors of an MLP layer on `rows` rows per group: output and statistics in `b`, one [rows][N] block per group ...
DenseLnIo mlp_io(const DenseLn& L, const float* x, long ldx, const LayerBuf& b, int rows) {   // ... on one input shared by the groups
  return DenseLnIo{x, ldx, 0, b.h, L.N, (long)rows * L.N, b.xhat, b.rstd};
}
DenseLnIo mlp_io(const DenseLn& L, const LayerBuf& below, const LayerBuf& b, int rows) {   // ... every group on its block of the layer below
  return DenseLnIo{below.h, L.K, L.groups > 1 ? (long)rows * L.K : 0, b.h, L.N, (long)rows * L.N, b.xhat, b.rstd};
}
// ... and of its backward pass: dy arrives in the layer's own scratch (dy_here), or is formed inside the LayerNorm backward
DenseLnGrad mlp_grad(const DenseLn& L, const GradBuf& s, int rows, bool dy_here = true) {
  return DenseLnGrad{dy_here ? s.dy : nullptr, L.N, (long)rows * L.N, s.dpre, s.dg};
}

// Layer L forward on `rows` rows per group for n independent instances of identical shape (instance i: parameters and tensors of
// job i, split-K scratch slabs_lane[i]): one grouped GEMM launch, K-split `smax` deep at the most, and one LayerNorm launch.
struct RowDot { const float *w, *b; float* out; long w_gs, b_gs; };   // rider of the LayerNorm launch: out[row] = y . w + b (critic head); *_gs: per-group heads, 0 = shared
struct LayerJob { const float* P; DenseLnIo t; RowDot dot; DenseLnDrop drop; };   // drop: the evaluation's Dropout site (zero: train=False)
int dense_ln_multi(serl_agent* a, const DenseLn& L, const LayerJob* jobs, int n, int rows, int smax, hipStream_t st) {
  SERL_REQUIRE(n >= 1 && n <= 3, "bad dense instance count");
  const int splitk = split_for(a->split_budget, rows, L.N, L.groups * n, smax);
  SERL_REQUIRE((long)L.groups * splitk * rows * L.N <= a->slabs_cap,
               "Dense layer: %d groups x %d K-splits x %d rows x width %d exceeds the slab scratch of %ld floats", L.groups, splitk,
               rows, L.N, a->slabs_cap);
  GemmDesc gd[3];
  LnFwdArgs lv[3];
  for (int i = 0; i < n; ++i) {
    const LayerJob& j = jobs[i];
    gd[i] = layer_fwd(L, j.P, j.t, rows, a->slabs_lane[i], splitk);
    lv[i] = layer_ln_fwd(L, j.P, j.t, rows, gd[i], j.drop);
    lv[i].dot_w = j.dot.w; lv[i].dot_b = j.dot.b; lv[i].dot_out = j.dot.out;
    lv[i].dot_gstride = j.dot.w_gs; lv[i].dot_b_gstride = j.dot.b_gs;
  }
  RC(gemm_f32_multi(gd, n, st));
  return ln_fwd_multi(lv, n, L.N, st);
}

// Policy forward + tanh-Gaussian sample (actor_critic_nets.py:179-227) for n independent inputs
struct PolJob {
  const float* P; PolBuf* pb;
  const float* enc; long ld_enc;
  const float* eps;
  float* act_out; long ld_act;
  float* sum_logp;
  float* alpha_out;  // optional rider: alpha = softplus(lagrange) of P (lagrange.py:49-50)
  // fused chain, eps == nullptr: the draws are hashed inside the head kernel from (eps_seed, global row) and kept in eps_out
  float* eps_out = nullptr; uint64_t eps_seed = 0; long eps_row0 = 0;
  const uint32_t* tf_key = nullptr; long tf_rows = 0, tf_row0 = 0;   // jax.random.normal(tf_key, (tf_rows, A)) rows tf_row0.. (serl_noise key_eps_*)
  DenseLnDrop drop[kL] = {};   // the Dropout sites of the MLP's layers (zero: train=False)
};
// the policy MLP of n instances, layer by layer (a GEMM and a LayerNorm launch each), into every job's buffers
int policy_mlp_multi(serl_agent* a, const PolJob* jobs, int n, int cnt, hipStream_t st) {
  const Offs& o = a->o;
  for (int l = 0; l < o.na; ++l) {
    LayerJob d[3];
    for (int i = 0; i < n; ++i) {
      const PolJob& j = jobs[i];
      MlpBuf& m = j.pb->m;
      d[i] = LayerJob{j.P, l ? mlp_io(o.a[l], m.l[l - 1], m.l[l], cnt) : mlp_io(o.a[0], j.enc, j.ld_enc, m.l[0], cnt), {}, j.drop[l]};
    }
    RC(dense_ln_multi(a, o.a[l], d, n, cnt, policy_smax(l), st));
  }
  return SERL_OK;
}
// The distance between the groups of the policy head's GEMMs (mean -> log_std, bias to bias); unused with one group, where it is
// A: the distance from the mean's bias to log_stds when there is such a leaf
inline long head_stride(const serl_agent* a) { return a->o.a_bs >= 0 ? a->o.a_bs - a->o.a_bm : a->cfg.act_dim; }
// What the head kernels read as `bias_ls` in the parameter vector P: the log-std bias, log_stds, or the agent's fixed_std
inline const float* head_bias_ls(const serl_agent* a, const float* P) { return a->o.a_bs >= 0 ? P + a->o.a_bs : a->fixed_std_dev; }
int policy_fwd_multi(serl_agent* a, const PolJob* jobs, int n, int cnt, hipStream_t st) {
  const serl_agent_cfg& c = a->cfg;
  const Offs& o = a->o;
  const int Hd = o.a[o.na - 1].N, A = c.act_dim;   // the head reads the last layer
  SERL_REQUIRE(n >= 1 && n <= 3, "bad policy instance count");
  GemmDesc gd[3];
  PolicyDistArgs pv[3];
  for (int i = 0; i < n; ++i) {
    const PolJob& j = jobs[i];
    const float* P = j.P;
    PolBuf& pb = *j.pb;
    // The head is no Dense -> LayerNorm layer (no LayerNorm): (mean, log_std) as two groups of one GEMM, the mean alone when log_stds is
    // a parameter vector (the stride is then unused)
    gd[i] = gemm_fwd(pb.m.l[o.na - 1].h, Hd, 0, P + o.a_Wm, head_stride(a), a->slabs_lane[i], a->head_groups, cnt, A, Hd, 4);
    pv[i] = PolicyDistArgs{};
    pv[i].mode = a->pol_mode;
    pv[i].slabs = a->slabs_lane[i]; pv[i].S = 4; pv[i].bias_mean = P + o.a_bm; pv[i].bias_ls = head_bias_ls(a, P); pv[i].pre = pb.pre;
    pv[i].eps = j.eps; pv[i].act = j.act_out; pv[i].ld_act = j.ld_act; pv[i].logp = pb.logp; pv[i].std_out = pb.std;
    pv[i].sum_logp = j.sum_logp; pv[i].lam = P + o.lam; pv[i].alpha_out = j.alpha_out;
  }
  RC(policy_mlp_multi(a, jobs, n, cnt, st));
  if (a->fuse) {   // the tanh-Gaussian head inside the head GEMM: last arriver of every 64-row tile (heads.hip, kEpiPolicy)
    SERL_REQUIRE(A <= 64, "the fused policy-head epilogue holds one 64-wide slab row per sample (act_dim %d)", A);
    SERL_REQUIRE(cdiv(cnt, 64) <= kCtrPerLane && 8 * pad64(cnt) * 64 <= a->slabs_cap, "policy head exceeds the fused epilogue's scratch");
    for (int i = 0; i < n; ++i) {
      const PolJob& j = jobs[i];
      GemmDesc& g = gd[i];
      g.ldc = 64; g.sCz = pad64(cnt) * 64;
      g.epi = kEpiPolicy; g.ctr = a->ctr + (long)i * kCtrPerLane;
      g.pd = pv[i];
      g.pd.sum_logp = nullptr;
      g.pd.eps_out = j.eps_out; g.pd.seed = j.eps_seed; g.pd.row_offset = j.eps_row0;
      g.pd.tf = j.tf_key ? 1 : 0;
      if (j.tf_key) { g.pd.tf_key[0] = j.tf_key[0]; g.pd.tf_key[1] = j.tf_key[1]; g.pd.tf_rows = j.tf_rows; g.pd.tf_row0 = j.tf_row0; }
      g.pd.B = cnt; g.pd.A = A; g.pd.std_min = c.std_min; g.pd.std_max = c.std_max;
      g.pd.slab_ld = g.ldc; g.pd.slab_stride = g.sCz;
      SERL_REQUIRE(j.eps || j.eps_out, "policy noise: neither draws nor a buffer for hashed ones");
      if (j.sum_logp) {   // sum_b log pi: a vector-sum job of the phase's deferred column-sum launch
        SERL_REQUIRE(a->pg_defer && a->pg_ncs < kMaxColsum, "no room for the log-prob sum job");
        a->pg_cs[a->pg_ncs++] = Colsum3Args{j.pb->logp, nullptr, nullptr, 1, cnt, 1, nullptr, j.sum_logp, nullptr, 0, 2};
      }
    }
    return gemm_f32_multi(gd, n, st);
  }
  RC(gemm_f32_multi(gd, n, st));
  return policy_dist_fwd_multi(pv, n, cnt, A, c.std_min, c.std_max, st);
}

// Critic ensemble forward on x = [enc | action] (actor_critic_nets.py:56-73, drq.py:201-207) for n independent
// (parameters, input) pairs; the shared Q head is fused into the LN kernel of the last layer
struct CritJob { const float* P; CritBuf* cb; DenseLnDrop drop[kL]; };   // drop: the Dropout sites of the layers (zero: train=False)
int critic_fwd_multi(serl_agent* a, const CritJob* jobs, int n, int cnt, hipStream_t st) {
  const Offs& o = a->o;
  SERL_REQUIRE(n >= 1 && n <= 3, "bad critic instance count");
  for (int l = 0; l < o.nc; ++l) {
    LayerJob d[3];
    for (int i = 0; i < n; ++i) {
      const float* P = jobs[i].P;
      CritBuf& cb = *jobs[i].cb;
      d[i] = LayerJob{P, l ? mlp_io(o.c[l], cb.m.l[l - 1], cb.m.l[l], cnt) : mlp_io(o.c[0], cb.x, a->XA, cb.m.l[0], cnt), {}, jobs[i].drop[l]};
      if (l == o.nc - 1)   // Q = h . w + b rides on the last layer's LayerNorm launch (a one-layer critic: on its only one)
        d[i].dot = RowDot{P + o.c_hw, P + o.c_hb, cb.q, a->state_only ? o.c[l].N : 0, a->state_only ? 1 : 0};
    }
    RC(dense_ln_multi(a, o.c[l], d, n, cnt, critic_smax(l), st));
  }
  return SERL_OK;
}

int flush_param_grads(serl_agent* a, hipStream_t st) {
  if (a->pg_ncs) RC(colsum3_multi(a->pg_cs, a->pg_ncs, st));
  if (a->pg_nwg) RC(gemm_f32_multi(a->pg_wg, a->pg_nwg, st));
  a->pg_ncs = a->pg_nwg = 0;
  return SERL_OK;
}

// A weight-gradient GEMM (written in place: splitk == 1): a job of the phase's deferred launch, or issued now
int wgrad(serl_agent* a, const GemmDesc& g, hipStream_t st) {
  if (a->pg_defer && a->pg_nwg < kMaxGemmGroups) {
    a->pg_wg[a->pg_nwg++] = g;  // issued by flush_param_grads
    return SERL_OK;
  }
  return gemm_f32(g, st);
}

// Backward of layer L through activation and LayerNorm: dpre and dg from dy, and with G (a gradient vector indexed like P) the
// gradients of its bias, scale and shift (a column-sum job) and of its kernel.  `head`: the riders of the critic's layer 2.
struct HeadDq {   // dy[row][col] = dq[row] * w[col] formed in the launch (rank-1); dq from `dq`, else from the `loss` rider, else dq_const
  const float* dq; const float* w; float dq_const; long w_gs; const LossArgs* loss;
};
int dense_ln_bwd(serl_agent* a, const DenseLn& L, const float* P, const DenseLnIo& t, const DenseLnGrad& d, int rows, float* G,
                 hipStream_t st, const HeadDq* head = nullptr, const DenseLnDrop& site = DenseLnDrop{}) {
  LnBwdArgs l = layer_ln_bwd(L, P, t, d, rows, site);
  if (head) { l.dq = head->dq; l.dq_w = head->w; l.dq_const = head->dq_const; l.dq_w_gstride = head->w_gs; }
  if (head && head->loss) {   // the critic loss rides on this launch and every row derives its dQ from the loss arguments (no critic_loss launch)
    l.dq_inline = 1;
    RC(ln_bwd_multi(&l, 1, *head->loss, st));
  } else {
    RC(ln_bwd(l, st));
  }
  if (!G) return SERL_OK;
  const Colsum3Args cs = layer_colsum(L, t, d, rows, G);
  if (a->pg_defer && a->pg_ncs < kMaxColsum) a->pg_cs[a->pg_ncs++] = cs;
  else RC(colsum3_multi(&cs, 1, st));
  return wgrad(a, layer_wgrad(L, t, d, rows, G), st);
}

// ---- the places where the two schedules of the update chain differ: a->fuse is read here and in
// policy_fwd_multi / encode_multi, nowhere in the phases themselves ----------------------------------------------------------

// dX = sum_g dY[g] * W[g]^T: `g` is the input-gradient GEMM (layer_igrad / gemm_igrad) without a place to land, which this
// gives it.  Fused: the per-group products go to padded scratch slabs and the last workgroup to arrive at an output tile adds
// them in group order (heads.hip, kEpiReduce).  Else: the products as slabs, then reduce_slabs.
int igrad_sum(serl_agent* a, GemmDesc g, float* out, long ldo, hipStream_t st) {
  const int groups = g.nbatch, rows = g.M, Kin = g.N;
  g.C = a->slabs;
  if (!a->fuse) {
    g.ldc = Kin; g.sCz = (long)rows * Kin;
    RC(gemm_f32(g, st));
    return reduce_slabs(a->slabs, groups, (long)rows * Kin, 1, rows, Kin, nullptr, 0, out, ldo, 0, false, st);
  }
  g.ldc = pad64(Kin); g.sCz = pad64(rows) * g.ldc;
  g.epi = kEpiReduce; g.zred = groups; g.ctr = a->ctr; g.out = out; g.ld_out = ldo; g.out_gstride = 0;
  SERL_REQUIRE((long)cdiv(rows, 64) * cdiv(Kin, 64) <= kCtrPerLane && groups * g.sCz <= a->slabs_cap,
               "input gradient: %d groups x %d rows x %d columns exceeds the fused epilogue's slab scratch of %ld floats, or its tiles the %d "
               "arrival counters", groups, rows, Kin, a->slabs_cap, kCtrPerLane);
  return gemm_f32(g, st);
}

// Gradient of the critic's head kernel: dw[j] = sum_{e,b} dq h2 for the shared head, dw[e][j] = sum_b dq[e][b] h2[e][b][j] with
// one head per member (state-only SAC): dq as one row [1][K] times h2.  A K above 1024 is split.  Fused: a deferred GEMM whose
// slabs the last arriver sums.  Else: the GEMM now, then reduce_slabs.  (M = 1: hand-filled, sAm is the schedule's own.)
int head_kernel_grad(serl_agent* a, CritBuf& cb, int cnt, hipStream_t st) {
  const int Hd = a->o.c[a->o.nc - 1].N, N = a->cfg.ensemble;   // the head reads the last layer
  const int groups = a->state_only ? N : 1, K = a->state_only ? cnt : N * cnt, split = K <= 1024 ? 1 : (a->state_only ? 4 : 8);
  float* out = a->Gc + a->o.c_hw;
  GemmDesc g{};
  g.A = a->dq; g.sAm = a->fuse ? 1 : 0; g.sAk = 1; g.sAb = a->state_only ? cnt : 0;
  g.B = cb.m.l[a->o.nc - 1].h; g.sBk = Hd; g.sBn = 1; g.sBb = a->state_only ? (long)cnt * Hd : 0;
  g.C = split == 1 ? out : a->slabs; g.ldc = Hd; g.sCz = Hd;   // (short K: written in place)
  g.M = 1; g.N = Hd; g.K = K; g.nbatch = groups; g.splitk = split;
  if (!a->fuse) {
    RC(gemm_f32(g, st));
    return split == 1 ? SERL_OK : reduce_slabs(a->slabs, split, Hd, groups, 1, Hd, nullptr, 0, out, Hd, a->state_only ? Hd : 0, false, st);
  }
  if (split > 1) {
    g.sCz = 64L * Hd;
    g.epi = kEpiReduce; g.zred = split; g.ctr = a->ctr; g.out = out; g.ld_out = Hd; g.out_gstride = Hd;
    SERL_REQUIRE((long)groups * split * g.sCz <= a->slabs_cap && groups * cdiv(Hd, 64) <= kCtrPerLane,
                 "head gradient: %d groups x %d K-splits x 64 rows x width %d exceeds the slab scratch of %ld floats, or its %d tiles the %d "
                 "arrival counters", groups, split, Hd, a->slabs_cap, groups * cdiv(Hd, 64), kCtrPerLane);
  }
  SERL_REQUIRE(a->pg_defer && a->pg_nwg < kMaxGemmGroups, "no room for the deferred head-gradient GEMM");
  a->pg_wg[a->pg_nwg++] = g;
  return SERL_OK;
}

// REDQ target + critic loss (sac.py:142-191).  Fused: *rider = the arguments, for the LayerNorm-backward launch that consumes
// dQ to carry as a rider workgroup.  Else: the critic_loss launch, no rider.
int critic_loss_or_rider(serl_agent* a, const LossArgs& L, hipStream_t st, const LossArgs** rider) {
  *rider = nullptr;
  if (a->fuse) { *rider = &L; return SERL_OK; }
  return critic_loss(L.qt, L.q, L.reward, L.mask, L.sel, L.E, L.B, L.discount, L.inv_norm, L.y_out, L.dq, L.scalars, L.dbias, st,
                     L.per_member != 0, L.logp_next, L.alpha);
}

// Gradient of the policy's head biases (mean, log_std): the column sums of dpre.  Fused: a job of the phase's deferred
// column-sum launch.  Else: a colsum launch.
// (kPolUniform: the second slab of dpre is the per-row gradient of the shared log_stds, whose leaf sits out_gstride = A behind
// the mean's bias: the same two column sums.  kPolFixed: dpre has no second slab and the std no leaf: the mean's sum alone.)
int head_bias_grad(serl_agent* a, int cnt, float* out, long out_gstride, hipStream_t st) {
  const int A = a->cfg.act_dim;
  const int groups = a->opts.std_param == SERL_STD_FIXED ? 1 : 2;
  if (!a->fuse) return colsum(a->dpre, nullptr, groups, cnt, A, out, out_gstride, false, st);
  SERL_REQUIRE(a->pg_ncs < kMaxColsum, "no room for the head-bias gradient job");
  a->pg_cs[a->pg_ncs++] = Colsum3Args{a->dpre, nullptr, nullptr, groups, cnt, A, nullptr, out, nullptr, out_gstride, 1};
  return SERL_OK;
}

// Critic backward down to dx [cnt][E+A]; parameter grads into Gc when `pg`.  The gradient wrt Q [ens][cnt] is the dq of the
// critic loss `loss` (critic phase), or the constant `dq_const` for every element (actor loss, loss == nullptr).
// `sites`: the layers' Dropout sites of the forward pass whose activations `cb` holds.
int critic_bwd(serl_agent* a, const float* P, CritBuf& cb, int cnt, bool pg, hipStream_t st, const LossArgs* loss, float dq_const,
               const DenseLnDrop* sites) {
  const Offs& o = a->o;
  float* G = pg ? a->Gc : nullptr;
  const LossArgs* rider = nullptr;
  if (loss) RC(critic_loss_or_rider(a, *loss, st, &rider));
  if (pg) RC(head_kernel_grad(a, cb, cnt, st));
  const int top = o.nc - 1;
  // the last layer: the gradient through the head dh = dq (x) w is formed inside the LN backward kernel (rank-1 mode), with the
  // critic-loss rider on the same launch; a one-layer critic has both on the layer that also feeds dx
  const HeadDq head{loss ? loss->dq : nullptr, P + o.c_hw, dq_const, a->state_only ? o.c[top].N : 0, rider};
  for (int l = top; l >= 0; --l) {
    const DenseLnGrad d = mlp_grad(o.c[l], a->s[l], cnt, l != top);
    const DenseLnIo t = l ? mlp_io(o.c[l], cb.m.l[l - 1], cb.m.l[l], cnt) : mlp_io(o.c[0], cb.x, a->XA, cb.m.l[0], cnt);
    RC(dense_ln_bwd(a, o.c[l], P, t, d, cnt, G, st, l == top ? &head : nullptr, sites[l]));
    if (l) RC(gemm_f32(layer_igrad(o.c[l], P, d, cnt, mlp_grad(o.c[l - 1], a->s[l - 1], cnt)), st));
    else return igrad_sum(a, layer_igrad(o.c[0], P, d, cnt, nullptr, 0, 0), a->dx, a->XA, st);   // dx = sum_e da1[e] * W1[e]^T
  }
  return SERL_OK;
}

// The critic path's backward below dx: d_enc = dx[:, :E] -> the proprio branch and the camera heads (LayerNorm, Dense, SLE
// kernel or the SmallEncoder's convs), into Gc.  `event_bucket0`: see serl_agent_critic_grads_bucketed.
// Fused: the LayerNorm backward of the camera heads (width 256) and of the proprio branch (width 64) share ONE launch in front
// of the event, and the SpatialLearnedEmbeddings gradient sums its batch splits itself (sle_bwd_fused).  Else: the proprio
// LayerNorm backward in front of the event, the camera heads' behind it, sle_bwd + reduce_slabs.
int enc_bwd_critic(serl_agent* a, const float* P, EncBuf& e, int off, int cnt, hipStream_t st, void* event_bucket0) {
  const serl_agent_cfg& c = a->cfg;
  const Offs& o = a->o;
  // both layers read their dy where the critic's backward left it: the cameras' column slices of dx, the proprio columns behind
  const DenseLnIo tc = cam_io(a, e), tp = a->prop || a->state_only ? prop_io(a, e, a->cur.state + (long)off * c.state_dim) : DenseLnIo{};
  const DenseLnGrad dc{a->dx, a->XA, o.cam.N, a->scam.dpre, a->scam.dg};
  const DenseLnGrad dp{a->dx + (long)c.n_cam * o.cam.N, a->XA, 0, a->sprop.dpre, a->sprop.dg};   // (unused without the proprio branch)
  if (!a->prop && !a->state_only) {   // image-only: the camera heads' LayerNorm backward alone, nothing of a proprio branch deferred
    if (a->fuse) {
      RC(ln_bwd(layer_ln_bwd(o.cam, P, tc, dc, cnt), st));
      SERL_REQUIRE(a->pg_defer && a->pg_ncs + 1 <= kMaxColsum, "no room for the deferred LayerNorm gradients");
      a->pg_cs[a->pg_ncs++] = layer_colsum(o.cam, tc, dc, cnt, a->Gc);
    }   // (un-fused: nothing in front of the event; the camera heads' dense_ln_bwd below runs their LayerNorm backward)
  } else if (a->fuse && !a->state_only) {
    LnBwdArgs lb[2] = {layer_ln_bwd(o.cam, P, tc, dc, cnt), layer_ln_bwd(o.prop, P, tp, dp, cnt)};
    RC(ln_bwd_multi(lb, 2, LossArgs{}, st));
    SERL_REQUIRE(a->pg_defer && a->pg_ncs + 2 <= kMaxColsum, "no room for the deferred LayerNorm gradients");
    a->pg_cs[a->pg_ncs++] = layer_colsum(o.prop, tp, dp, cnt, a->Gc);
    a->pg_cs[a->pg_ncs++] = layer_colsum(o.cam, tc, dc, cnt, a->Gc);
    RC(wgrad(a, layer_wgrad(o.prop, tp, dp, cnt, a->Gc), st));
  } else if (!a->state_only) {
    RC(dense_ln_bwd(a, o.prop, P, tp, dp, cnt, a->Gc, st));
  }
  if (event_bucket0) {   // bucket 0 (ensemble | head | proprio, where the agent has the branch | scalars) is final once the jobs deferred so far have run
    RC(flush_param_grads(a, st));
    SERL_HIP(hipEventRecord((hipEvent_t)event_bucket0, st));
  }
  if (a->state_only) return SERL_OK;
  if (a->fuse) RC(wgrad(a, layer_wgrad(o.cam, tc, dc, cnt, a->Gc), st));
  else RC(dense_ln_bwd(a, o.cam, P, tc, dc, cnt, a->Gc, st));
  RC(gemm_f32(layer_igrad(o.cam, P, dc, cnt, a->df, a->D, (long)cnt * a->D), st));
  if (a->small)   // through the average pool and the four convs of the forward pass that ran last (theta at observations)
    return small_backward(a->sws, P, o.enc0, o.cam_stride, c.n_cam, cnt, a->df, (long)cnt * a->D, a->Gc, st);
  // dK of every camera: partial sums over batch splits (grid.z = camera x batch split), summed by the last arriver or a reduction
  const long sle_n = (long)a->HW * 512 * c.sle_features;
  const float* x = a->feats + (long)off * a->HW * 512;
  if (a->fuse) {
    SERL_REQUIRE((long)c.n_cam * a->HW * 2 <= kCtrPerLane, "SLE gradient exceeds the arrival counters");
    return sle_bwd_fused(x, a->df, a->sle_part, cnt, a->HW, 512, kSleSplit, c.n_cam, (long)c.batch * a->HW * 512, (long)cnt * a->D,
                         (long)kSleSplit * sle_n, a->Gc + o.enc0, o.cam_stride, a->ctr, st);
  }
  RC(sle_bwd(x, a->df, a->sle_part, cnt, a->HW, 512, kSleSplit, c.n_cam, (long)c.batch * a->HW * 512,
             (long)cnt * a->D, (long)kSleSplit * sle_n, st));
  return reduce_slabs(a->sle_part, kSleSplit, sle_n, c.n_cam, 1, (int)sle_n, nullptr, 0, a->Gc + o.enc0, sle_n,
                      o.cam_stride, false, st);
}

// rows of the GLOBAL (mini)batch in front of this rank's `cnt` rows (serl_agent_set_shard: this rank owns rows shard_off.. of a
// global batch of shard_global; a minibatch of a high-UTD update is sharded the same way)
static long tf_row0_of(const serl_agent* a, int cnt) {
  return a->shard_global ? (a->shard_off * (long)cnt) / std::max<long>(a->cur.batch, 1) : 0;
}

// Noise of one policy evaluation and of the encoder pass that feeds it: the normal draws eps [B][A] and the Dropout keep-mask
// [n_cam][B][D].  Each is a caller-provided tensor (parity mode), drawn from a jax.random key (serl_noise key_*, host words), or
// hashed from a seed of the agent's own stream -- in that order of preference.
struct PhaseNoise {
  const float* eps; float* eps_out;        // eps == nullptr: drawn into eps_out from tf_eps, or else from eps_seed
  const uint32_t* tf_eps; uint64_t eps_seed;
  const uint8_t* mask; uint8_t* mask_out;  // mask == nullptr: gen_mask 0 = no Dropout, 1 = hashed from mask_seed, 2 = drawn from tf_mask
  int gen_mask; const uint32_t* tf_mask; uint64_t mask_seed;
};
// The one place that advances the agent's noise stream: a seed is taken for eps, then for the mask, where neither tensor nor key
// is given (no Dropout without the SLE branch).  Buffers of `slot`.
PhaseNoise draw_noise(serl_agent* a, const float* given_eps, const uint8_t* given_mask, int slot, const uint32_t* key_eps,
                      const uint32_t* key_mask) {
  const serl_agent_cfg& c = a->cfg;
  PhaseNoise z{};
  z.eps = given_eps; z.eps_out = a->eps_buf[slot];
  z.mask_out = a->mask_buf[slot];
  if (!given_eps) {
    if (key_eps) z.tf_eps = key_eps;
    else z.eps_seed = c.seed ^ (0xA5A5ull + 7919ull * (++a->noise_ctr));
  }
  if (given_mask || a->state_only || a->small) z.mask = a->small ? nullptr : given_mask;
  else if (key_mask) { z.gen_mask = 2; z.tf_mask = key_mask; }
  else { z.gen_mask = 1; z.mask_seed = c.seed ^ (0x5A5Aull + 104729ull * (++a->noise_ctr)); }
  return z;
}
// Fused: nothing is generated ahead of time -- missing normal draws are made inside the policy-head epilogue and kept in eps_out,
// a missing Dropout mask inside the SLE kernel.  Else: the n descriptors of a phase are materialised first and left as given
// tensors: key draws by serl_jax_fill (rows [off, off + cnt) of the buffers = rows tf_row0.. of the global arrays), seeded ones
// for the whole batch by ONE gen_noise_multi launch (same hash: seed and global-row indexing as in the fused kernels).
int materialise_noise(serl_agent* a, PhaseNoise* v, int n, int off, int cnt, long global_count, hipStream_t st) {
  if (a->fuse) return SERL_OK;
  const serl_agent_cfg& c = a->cfg;
  const long rows = a->cur.batch, row0 = tf_row0_of(a, cnt);
  NoiseJob gen[kMaxMulti];
  int ngen = 0;
  for (int i = 0; i < n; ++i) {
    PhaseNoise& z = v[i];
    serl_jax_job jobs[1 + SERL_MAX_CAMS];
    int nj = 0;
    if (!z.eps && z.tf_eps) {
      serl_jax_job& j = jobs[nj++];
      j = serl_jax_job{};
      j.key[0] = z.tf_eps[0]; j.key[1] = z.tf_eps[1]; j.kind = SERL_JAX_NORMAL;
      j.n_total = global_count * c.act_dim; j.first = row0 * c.act_dim; j.count = (long)cnt * c.act_dim;
      j.out = z.eps_out + (long)off * c.act_dim;
    } else if (!z.eps) {
      gen[ngen++] = NoiseJob{z.eps_out, rows * c.act_dim, z.eps_seed, 0, 0.f, rows, a->shard_global, a->shard_off, c.act_dim};
    }
    for (int k = 0; k < c.n_cam && z.gen_mask == 2; ++k) {
      serl_jax_job& j = jobs[nj++];
      j = serl_jax_job{};
      j.key[0] = z.tf_mask[2 * k]; j.key[1] = z.tf_mask[2 * k + 1]; j.kind = SERL_JAX_BERNOULLI_U8; j.p = 1.0f - c.dropout;
      j.n_total = global_count * a->D; j.first = row0 * a->D; j.count = (long)cnt * a->D;
      j.out = z.mask_out + ((long)k * rows + off) * a->D;
    }
    if (z.gen_mask == 1)
      gen[ngen++] = NoiseJob{z.mask_out, (long)c.n_cam * rows * a->D, z.mask_seed, 1, 1.0f - c.dropout, rows, a->shard_global, a->shard_off, a->D};
    if (nj) RC(serl_jax_fill(c.device, jobs, nj, (void*)st));
    z = PhaseNoise{z.eps ? z.eps : z.eps_out, z.eps_out, nullptr, 0, z.gen_mask ? z.mask_out : z.mask, z.mask_out, 0, nullptr, 0};
  }
  return ngen ? gen_noise_multi(gen, ngen, st) : SERL_OK;
}
// hands the noise of a phase's rows [off, off + cnt) (= rows tf_row0_of.. of the global_count rows a key draws) to its jobs
void set_noise(const serl_agent* a, EncJob& e, PolJob& p, const PhaseNoise& z, long off, int cnt, long global_count) {
  const int A = a->cfg.act_dim;
  const long tf_row0 = tf_row0_of(a, cnt);
  e.mask = z.mask; e.gen_mask = z.gen_mask; e.mask_seed = z.mask_seed;
  e.tf_key = z.tf_mask; e.tf_rows = global_count; e.tf_row0 = tf_row0;
  p.eps = z.eps ? z.eps + off * A : nullptr;
  p.eps_out = z.eps_out + off * A; p.eps_seed = z.eps_seed; p.eps_row0 = a->shard_off + off;
  p.tf_key = z.tf_eps; p.tf_rows = global_count; p.tf_row0 = tf_row0;
}

// The Dropout sites of the layers of MLP evaluation `site` (SERL_SITE_*) on rows [off, off + cnt) of the selected batch, at
// rate `rate` (0: nothing is read and the agent's noise stream does not move -- a rate-0 agent draws what it always drew).  Each
// layer: the bound mask, else the bound key (`key_row`: the critic update of a high-UTD call, for the critic-loss sites), else a
// seed of the agent's own stream, one per (site, layer) in call order, which every rank of a data-parallel job takes alike.
void mlp_sites(serl_agent* a, int site, double rate, int off, int cnt, long global_count, int key_row, DenseLnDrop (&out)[kL]) {
  for (DenseLnDrop& d : out) d = DenseLnDrop{};
  if (!(rate > 0.0)) return;
  const serl_mlp_noise& z = a->mlp_cur;
  const bool critic = site == SERL_SITE_Q_TARGET || site == SERL_SITE_Q_ONLINE || site == SERL_SITE_Q_ACTOR;
  const serl_mlp_opts& net = critic ? a->opts.critic : a->opts.policy;
  const int* dims = net.dims;
  const int n = net.n_layers;
  long below = 0;   // mask elements per batch row of the layers in front of layer l
  for (int l = 0; l < n; below += dims[l], ++l) {
    DenseLnDrop& d = out[l];
    d.train = 1;
    if (z.mask[site]) d.mask = z.mask[site] + below * a->cur.batch + (long)off * dims[l];
    else if (z.key[site]) { d.key = z.key[site] + ((long)key_row * n + l) * 2; d.key_rows = global_count; d.key_row0 = tf_row0_of(a, cnt); }
    else { d.seed = a->cfg.seed ^ (0xD0D0ull + 15485863ull * (++a->noise_ctr)); d.hash_row0 = a->shard_off + off; }
  }
}
// the bound mask tensors are laid out for the rows of the selected batch
int mlp_masks_fit(const serl_agent* a) {
  for (int s = 0; s < SERL_MLP_SITES; ++s)
    SERL_REQUIRE(!a->mlp_cur.mask[s] || a->mlp_cur.mask_rows == a->cur.batch,
                 "serl_mlp_noise: the masks of site %d hold %d rows per layer, the batch has %d", s, a->mlp_cur.mask_rows, a->cur.batch);
  return SERL_OK;
}
// The outermost update / phase / dry-run entry point takes the serl_agent_set_mlp_noise binding; the entry points it calls read
// the same one; when it returns, on every path, the binding is gone.
struct MlpNoiseScope {
  serl_agent* a;
  explicit MlpNoiseScope(serl_agent* a_) : a(a_) {
    if (a && a->mlp_depth++ == 0) { a->mlp_cur = a->mlp_bound; a->mlp_bound = serl_mlp_noise{}; }
  }
  ~MlpNoiseScope() {
    if (a && --a->mlp_depth == 0) a->mlp_cur = serl_mlp_noise{};
  }
};

// learning rate of optimizer `tx` at `count` (optimizers.py:14-30): warm-up -> constant, or warm-up -> cosine decay
float lr_at(const serl_agent_cfg& c, int64_t count, int tx) {
  const float peak = (c.tx_lr_set[tx] || c.tx_lr[tx] > 0.f) ? c.tx_lr[tx] : c.lr;
  int warm = (tx == SERL_TX_TEMPERATURE && c.temp_warmup_steps >= 0) ? c.temp_warmup_steps : c.warmup_steps;
  if (c.tx_warmup[tx] > 0) warm = c.tx_warmup[tx] - 1;
  if (count < warm) return (float)((double)peak * (double)count / (double)warm);   // linear_schedule(0, peak, warm)
  if (c.tx_cosine_steps[tx] > 0) {   // optax.warmup_cosine_decay_schedule(0, peak, warm, decay_steps, end_value = 0)
    const double T = (double)std::max(c.tx_cosine_steps[tx] - warm, 1);
    const double k = std::min((double)(count - warm), T);
    return (float)((double)peak * 0.5 * (1.0 + std::cos(M_PI * k / T)));
  }
  return peak;
}

}  // namespace

extern "C" {

static int create_agent(const serl_agent_cfg* cfg, const serl_agent_opts* opts, serl_agent** out);

int serl_agent_create_opts(const serl_agent_cfg* cfg, const serl_agent_opts* opts, serl_agent** out) {
  SERL_REQUIRE(cfg && opts && out, "NULL argument");
  return create_agent(cfg, opts, out);
}

// The entry points from before serl_agent_opts: each states its argument list as opts, the fields it has no argument for left 0.
// SERL_STD_FIXED came with serl_agent_create_fixed_std: the older ones keep refusing it, in the words they always used.
static int three_std_params(int std_param) {
  SERL_REQUIRE(std_param >= SERL_STD_EXP && std_param <= SERL_STD_UNIFORM,
               "std_param %d is not SERL_STD_EXP (0), SERL_STD_SOFTPLUS (1) or SERL_STD_UNIFORM (2)", std_param);
  return SERL_OK;
}

int serl_agent_create(const serl_agent_cfg* cfg, serl_agent** out) { return serl_agent_create_policy(cfg, SERL_STD_EXP, 0, out); }

int serl_agent_create_policy(const serl_agent_cfg* cfg, int std_param, int no_tanh, serl_agent** out) {
  return serl_agent_create_mlp(cfg, std_param, no_tanh, SERL_ACT_TANH, SERL_ACT_TANH, out);
}

int serl_agent_create_mlp(const serl_agent_cfg* cfg, int std_param, int no_tanh, int critic_act, int policy_act, serl_agent** out) {
  return serl_agent_create_dropout(cfg, std_param, no_tanh, critic_act, policy_act, 0.0, 0.0, out);
}

int serl_agent_create_dropout(const serl_agent_cfg* cfg, int std_param, int no_tanh, int critic_act, int policy_act, double critic_dropout,
                              double policy_dropout, serl_agent** out) {
  SERL_REQUIRE(cfg && out, "NULL argument");
  if (int rc = three_std_params(std_param)) return rc;
  serl_agent_opts o{};
  o.std_param = std_param; o.no_tanh = no_tanh;
  o.critic.act = critic_act; o.policy.act = policy_act;
  o.critic.dropout = critic_dropout; o.policy.dropout = policy_dropout;
  return create_agent(cfg, &o, out);
}

int serl_agent_create_shapes(const serl_agent_cfg* cfg, int std_param, int no_tanh, int critic_act, int policy_act,
                             const int* critic_dims, int n_critic, const int* policy_dims, int n_policy, serl_agent** out) {
  return serl_agent_create_layer_norm(cfg, std_param, no_tanh, critic_act, policy_act, critic_dims, n_critic, policy_dims, n_policy, 1, 1, out);
}

int serl_agent_create_layer_norm(const serl_agent_cfg* cfg, int std_param, int no_tanh, int critic_act, int policy_act,
                                 const int* critic_dims, int n_critic, const int* policy_dims, int n_policy, int critic_layer_norm,
                                 int policy_layer_norm, serl_agent** out) {
  if (int rc = three_std_params(std_param)) return rc;
  return serl_agent_create_fixed_std(cfg, std_param, no_tanh, critic_act, policy_act, critic_dims, n_critic, policy_dims, n_policy,
                                     critic_layer_norm, policy_layer_norm, nullptr, out);
}

int serl_agent_create_fixed_std(const serl_agent_cfg* cfg, int std_param, int no_tanh, int critic_act, int policy_act,
                                const int* critic_dims, int n_critic, const int* policy_dims, int n_policy, int critic_layer_norm,
                                int policy_layer_norm, const float* fixed_std, serl_agent** out) {
  SERL_REQUIRE(cfg && out, "NULL argument");
  SERL_REQUIRE(critic_dims && policy_dims, "%s is NULL: the hidden widths of the %s's MLP, 1 to %d of them",
               critic_dims ? "policy_dims" : "critic_dims", critic_dims ? "policy" : "critic", SERL_MAX_MLP_LAYERS);
  SERL_REQUIRE(critic_layer_norm == 0 || critic_layer_norm == 1, "critic_layer_norm %d is not 0 (no LayerNorm) or 1", critic_layer_norm);
  SERL_REQUIRE(policy_layer_norm == 0 || policy_layer_norm == 1, "policy_layer_norm %d is not 0 (no LayerNorm) or 1", policy_layer_norm);
  serl_agent_opts o{};
  o.std_param = std_param; o.no_tanh = no_tanh;
  o.critic.act = critic_act; o.policy.act = policy_act;
  o.fixed_std = fixed_std;
  for (int k = 0; k < 2; ++k) {
    serl_mlp_opts& net = k ? o.policy : o.critic;
    const int n = k ? n_policy : n_critic;
    // checked HERE, before anything is copied into dims[]; a caller's 0 is refused as 0 layers, it never becomes "use cfg->hidden"
    SERL_REQUIRE(n >= 1 && n <= SERL_MAX_MLP_LAYERS, "%s MLP: %d hidden layers (served: 1 to %d layers, each a multiple of 64 in [64, 1024] wide)",
                 k ? "policy" : "critic", n, SERL_MAX_MLP_LAYERS);
    net.n_layers = n;
    std::copy_n(k ? policy_dims : critic_dims, n, net.dims);
    net.no_layer_norm = !(k ? policy_layer_norm : critic_layer_norm);
  }
  return create_agent(cfg, &o, out);
}

// the vector the agent was given with SERL_STD_FIXED (before the clip)
int serl_agent_fixed_std(serl_agent* a, float* out) {
  SERL_REQUIRE(a && out, "NULL argument");
  SERL_REQUIRE(a->opts.std_param == SERL_STD_FIXED, "the agent's std parameterisation is %d, not SERL_STD_FIXED (3): it has no fixed_std", a->opts.std_param);
  std::copy(a->fixed_std.begin(), a->fixed_std.end(), out);
  return SERL_OK;
}

// mlp.py:29-30: whether the layers of an agent's critic (network 0) or policy (1) MLP have their LayerNorm
int serl_agent_mlp_layer_norm(serl_agent* a, int network) {
  if (!a || (network != 0 && network != 1)) return -1;
  return (network ? a->opts.policy : a->opts.critic).no_layer_norm ? 0 : 1;
}

// mlp.py:19-31; sac.py:516-524, drq.py:188-207: the hidden widths an agent was created with
int serl_agent_mlp_dims(serl_agent* a, int network, int dims[SERL_MAX_MLP_LAYERS]) {
  if (!a || !dims || (network != 0 && network != 1)) return -1;
  const serl_mlp_opts& net = network ? a->opts.policy : a->opts.critic;
  std::copy_n(a->true_dims[network], net.n_layers, dims);   // (net.dims: the storage widths)
  return net.n_layers;
}

// Every entry point's agent (serl_mi355.h, NETWORK OPTIONS).  The two networks are built from separate kwargs (sac.py:516-524,
// drq.py:188-207), so their options are independent: mlp.py:19-31 applies `activations` behind every layer and loops over
// hidden_dims of any length, :27-28 puts Dropout in front of the LayerNorm, :29-30 makes the LayerNorm optional;
// actor_critic_nets.py:189-192,212: with fixed_std, stds = clip(fixed_std, std_min, std_max), no Dense_1 and no log_stds.
static int create_agent(const serl_agent_cfg* cfg, const serl_agent_opts* opts, serl_agent** out) {
  const serl_mlp_opts &critic = opts->critic, &policy = opts->policy;
  const int std_param = opts->std_param;
  const float* fixed_std = opts->fixed_std;
  SERL_REQUIRE(critic.no_layer_norm == 0 || critic.no_layer_norm == 1, "critic no_layer_norm %d is not 0 (LayerNorm) or 1 (none)", critic.no_layer_norm);
  SERL_REQUIRE(policy.no_layer_norm == 0 || policy.no_layer_norm == 1, "policy no_layer_norm %d is not 0 (LayerNorm) or 1 (none)", policy.no_layer_norm);
  SERL_REQUIRE((!critic.no_layer_norm || !(critic.dropout > 0.0)) && (!policy.no_layer_norm || !(policy.dropout > 0.0)),
               "Dropout in an MLP without LayerNorm is not served");
  // (the keep probability float32(1 - rate) must itself lie below 1 and above 0)
  SERL_REQUIRE(critic.dropout >= 0.0 && (float)(1.0 - critic.dropout) > 0.f, "critic_dropout %g: a Dropout rate lies in [0, 1)", critic.dropout);
  SERL_REQUIRE(policy.dropout >= 0.0 && (float)(1.0 - policy.dropout) > 0.f, "policy_dropout %g: a Dropout rate lies in [0, 1)", policy.dropout);
  // what the argument lists could not say and opts can: Dropout is served where it always was
  if (critic.dropout > 0.0 || policy.dropout > 0.0) {
    // (the keep-masks and per-layer keys of serl_mlp_noise are laid out for two layers of cfg->hidden)
    SERL_REQUIRE(critic.n_layers == 0 && policy.n_layers == 0, "dropout %g / %g with n_layers %d / %d (critic / policy): Dropout is served with "
                 "n_layers 0 in both networks, two layers of cfg->hidden", critic.dropout, policy.dropout, critic.n_layers, policy.n_layers);
    SERL_REQUIRE(!critic.no_layer_norm && !policy.no_layer_norm, "dropout %g / %g with no_layer_norm %d / %d (critic / policy): Dropout is "
                 "served in agents whose two networks have their LayerNorm", critic.dropout, policy.dropout, critic.no_layer_norm, policy.no_layer_norm);
    SERL_REQUIRE(std_param != SERL_STD_FIXED, "dropout %g / %g (critic / policy) with std_param SERL_STD_FIXED (3): Dropout is served in "
                 "agents whose policy head has std leaves", critic.dropout, policy.dropout);
  }
  SERL_REQUIRE(cfg->n_cam >= 0 && cfg->n_cam <= SERL_MAX_CAMS, "n_cam %d not in [0,%d]", cfg->n_cam, SERL_MAX_CAMS);
  SERL_REQUIRE(opts->no_proprio == 0 || opts->no_proprio == 1, "no_proprio %d is not 0 (the proprio branch) or 1 (image codes alone)", opts->no_proprio);
  SERL_REQUIRE(!opts->no_proprio || cfg->n_cam > 0, "no_proprio 1 with n_cam 0: a state-only agent has no EncodingWrapper, its input is the state");
  if (opts->no_proprio && (critic.dropout > 0.0 || policy.dropout > 0.0)) {
    set_error("dropout %g / %g (critic / policy) with no_proprio 1: Dropout in the MLPs is served in agents with the proprio branch",
              critic.dropout, policy.dropout);
    return SERL_ERR_UNSUPPORTED;
  }
  SERL_REQUIRE(cfg->n_cam == 0 || (cfg->H >= 32 && cfg->W >= 32), "images must be at least 32x32");
  SERL_REQUIRE(cfg->encoder_type == SERL_ENCODER_RESNET_PRETRAINED || cfg->encoder_type == SERL_ENCODER_SMALL,
               "Unknown encoder type: %d", cfg->encoder_type);
  SERL_REQUIRE(cfg->n_cam > 0 || cfg->ensemble <= 16, "state-only SAC supports ensembles of at most 16");
  SERL_REQUIRE(opts->ragged_widths == 0 || opts->ragged_widths == 1, "ragged_widths %d is not 0 (widths on the 64 grid) or 1 (any width in [1, 1024])",
               opts->ragged_widths);
  // one wave owns a LayerNorm row and a lane holds hidden / 64 of its columns, 16 at the most (heads.hip).  ragged_widths 1: any
  // width in [1, 1024], a layer off the grid being stored 64 ceil(d / 64) wide in zero padding
  const bool ragged = opts->ragged_widths == 1;
  const auto width_ok = [&](int d) { return d <= 1024 && (ragged ? d >= 1 : d >= 64 && d % 64 == 0); };
  const char* served = ragged ? "served with ragged_widths 1: 1 to %d layers, each in [1, 1024] wide"
                              : "served: 1 to %d layers, each a multiple of 64 in [64, 1024] wide";
  bool off_grid = false;
  if (critic.n_layers == 0 || policy.n_layers == 0) {
    SERL_REQUIRE(width_ok(cfg->hidden), ragged ? "hidden must lie in [1, 1024] with ragged_widths 1 (got %d): the width of the critic's and the policy's two MLP layers"
                                               : "hidden must be a multiple of 64 in [64, 1024] (got %d): the width of the critic's and the policy's two MLP layers",
                 cfg->hidden);
    off_grid = cfg->hidden % 64 != 0;
  }
  for (const serl_mlp_opts* net : {&critic, &policy}) {
    if (net->n_layers == 0) continue;   // two layers of cfg->hidden, checked above
    const std::string name = net == &critic ? "critic" : "policy";
    SERL_REQUIRE(net->n_layers >= 1 && net->n_layers <= SERL_MAX_MLP_LAYERS, (name + " MLP: %d hidden layers (" + served + ")").c_str(), net->n_layers,
                 SERL_MAX_MLP_LAYERS);
    for (int j = 0; j < net->n_layers; ++j) {
      SERL_REQUIRE(width_ok(net->dims[j]), (name + " MLP: layer %d has width %d (" + served + ")").c_str(), j + 1, net->dims[j], SERL_MAX_MLP_LAYERS);
      off_grid = off_grid || net->dims[j] % 64 != 0;
    }
  }
  // (the jax-keyed keep-masks are laid out for [rows][h] with h on the grid; off_grid implies ragged here)
  SERL_REQUIRE(!off_grid || !(critic.dropout > 0.0 || policy.dropout > 0.0), "dropout %g / %g (critic / policy) beside an MLP width off the 64 grid "
               "under ragged_widths 1: Dropout is served at widths that are multiples of 64", critic.dropout, policy.dropout);
  SERL_REQUIRE(cfg->bottleneck == 256, "bottleneck must be 256 (got %d): the reference fixes bottleneck_dim=256 in create_drq", cfg->bottleneck);
  SERL_REQUIRE(cfg->proprio_dim == 64, "proprio_dim must be 64");
  SERL_REQUIRE(cfg->sle_features == 8, "sle_features must be 8");
  SERL_REQUIRE(cfg->batch >= 1 && cfg->ensemble >= 2 && cfg->state_dim >= 1 && cfg->act_dim >= 1 && cfg->act_dim <= 64, "bad dims");
  const int num_stack = cfg->num_stack > 0 ? cfg->num_stack : 1;   // 0 = 1: a zero-initialised field keeps its meaning
  SERL_REQUIRE(cfg->num_stack >= 0 && num_stack <= kSmallMaxStack, "num_stack %d not in [1,%d]", cfg->num_stack, kSmallMaxStack);
  if (num_stack > 1 && cfg->n_cam > 0 && cfg->encoder_type == SERL_ENCODER_RESNET_PRETRAINED) {
    set_error("num_stack %d with the pretrained ResNet-10: its conv_init kernel is (7,7,3,64), 3 input channels, and cannot be applied "
              "to the %d channels of a folded stack (common/encoding.py:39-44); frame stacks are served with SERL_ENCODER_SMALL", num_stack, 3 * num_stack);
    return SERL_ERR_UNSUPPORTED;
  }
  SERL_REQUIRE(num_stack == 1 || cfg->n_cam > 0, "num_stack %d on a state-only agent: its state path has no stacking wrapper", num_stack);
  SERL_REQUIRE(std_param >= SERL_STD_EXP && std_param <= SERL_STD_FIXED,
               "std_param %d is not SERL_STD_EXP (0), SERL_STD_SOFTPLUS (1), SERL_STD_UNIFORM (2) or SERL_STD_FIXED (3)", std_param);
  SERL_REQUIRE(std_param != SERL_STD_FIXED || fixed_std, "std_param SERL_STD_FIXED (3) needs fixed_std: act_dim floats, got NULL");
  SERL_REQUIRE(std_param == SERL_STD_FIXED || !fixed_std, "fixed_std is given with std_param %d: it goes with SERL_STD_FIXED (3) alone", std_param);
  for (int j = 0; fixed_std && j < cfg->act_dim; ++j)
    SERL_REQUIRE(std::isfinite(fixed_std[j]) && fixed_std[j] > 0.f, "fixed_std[%d] = %g is not a finite positive number", j, (double)fixed_std[j]);
  SERL_REQUIRE(opts->no_tanh == 0 || opts->no_tanh == 1, "no_tanh %d is not 0 (tanh-squashed) or 1 (plain Gaussian)", opts->no_tanh);
  SERL_REQUIRE(critic.act >= 0 && critic.act < kActCount, "critic_act %d: served are SERL_ACT_TANH (0), SERL_ACT_RELU (1) and SERL_ACT_SWISH (2)", critic.act);
  SERL_REQUIRE(policy.act >= 0 && policy.act < kActCount, "policy_act %d: served are SERL_ACT_TANH (0), SERL_ACT_RELU (1) and SERL_ACT_SWISH (2)", policy.act);
  SERL_REQUIRE(cfg->state_dim % num_stack == 0, "state_dim %d is not num_stack %d proprio vectors (state_dim is the flattened width T * S)",
               cfg->state_dim, num_stack);
  bool any_wd = false;
  for (int t = 0; t < 3; ++t) {
    // adamw decays EVERY leaf of the tree the optimizer is given (common.py:142-147 passes the full params): with the pretrained
    // trunk in that tree the agent runs in live-trunk mode (below)
    // (a decay of exactly 0 moves no leaf: such an agent keeps the frozen-trunk path, bit for bit)
    any_wd = any_wd || (cfg->tx_weight_decay_on[t] && cfg->tx_weight_decay[t] != 0.f);
    SERL_REQUIRE(cfg->tx_lr[t] >= 0.f && cfg->tx_warmup[t] >= 0 && cfg->tx_cosine_steps[t] >= 0 && cfg->tx_clip_norm[t] >= 0.f,
                 "bad optimizer options for optimizer %d", t);
  }
  SERL_HIP(hipSetDevice(cfg->device));
  serl_agent* a = new serl_agent();
  a->cfg = *cfg;
  a->cfg.num_stack = num_stack;
  a->opts = *opts;
  for (serl_mlp_opts* net : {&a->opts.critic, &a->opts.policy}) {
    if (net->n_layers == 0) { net->n_layers = 2; net->dims[0] = net->dims[1] = cfg->hidden; }
    std::fill(net->dims + net->n_layers, net->dims + kL, 0);
    int* td = a->true_dims[net == &a->opts.policy];
    for (int j = 0; j < kL; ++j) { td[j] = net->dims[j]; net->dims[j] = (int)pad64(td[j]); }   // (on the grid: the same number twice)
  }
  if (fixed_std) a->fixed_std.assign(fixed_std, fixed_std + cfg->act_dim);
  a->opts.fixed_std = fixed_std ? a->fixed_std.data() : nullptr;   // the caller's pointer is not kept
  { const char* e = getenv("SERL_CHAIN_FUSE"); a->fuse = !(e && e[0] == '0'); }
  build_layout(a);
  a->live = any_wd && a->trunk_count > 0;
  if (int rc = alloc_zeroed(&a->arena, carve(a, nullptr), "agent arena")) {
    delete a;
    return rc;
  }
  carve(a, a->arena);
  if (fixed_std) {   // a constant of the agent, outside the arena: nothing that walks the parameters meets it
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&a->fixed_std_dev), sizeof(float) * cfg->act_dim);
    if (e == hipSuccess) e = hipMemcpy(a->fixed_std_dev, fixed_std, sizeof(float) * cfg->act_dim, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      set_error("fixed_std: %s", hipGetErrorString(e));
      if (a->fixed_std_dev) (void)hipFree(a->fixed_std_dev);
      (void)hipFree(a->arena);
      delete a;
      return SERL_ERR_HIP;
    }
  }
  if (!a->state_only && !a->small) a->tw = trunk_weights(a->trunk, a->to);
  if (a->live) a->tw_t = trunk_weights(a->trunk_t, a->to);
  *out = a;
  return SERL_OK;
}

int serl_agent_live_trunk(serl_agent* a) { return a ? (a->live ? 1 : 0) : -1; }
int serl_agent_use_proprio(serl_agent* a) { return a ? (a->opts.no_proprio ? 0 : 1) : -1; }

int serl_agent_destroy(serl_agent* a) {
  if (!a) return SERL_OK;
  if (a->snapshots > 0) {   // their staging slots hold pointers into the arena freed below
    set_error("the agent has %d live snapshot handle(s): serl_snapshot_destroy them first", a->snapshots);
    return SERL_ERR_STATE;
  }
  (void)hipSetDevice(a->cfg.device);
  (void)hipDeviceSynchronize();
  if (a->arena) (void)hipFree(a->arena);
  if (a->fixed_std_dev) (void)hipFree(a->fixed_std_dev);
  delete a;
  return SERL_OK;
}

int serl_agent_num_leaves(serl_agent* a) {
  return a ? (int)(a->theta_leaves.size() + a->trunk_leaves.size()) : -1;
}

int serl_agent_leaf_info(serl_agent* a, int i, char* name_out, int name_cap, int64_t* count) {
  SERL_REQUIRE(a && name_out && count, "NULL argument");
  const int nt = (int)a->theta_leaves.size();
  SERL_REQUIRE(i >= 0 && i < serl_agent_num_leaves(a), "leaf index %d out of range", i);
  const Leaf& l = i < nt ? a->theta_leaves[i] : a->trunk_leaves[i - nt];
  snprintf(name_out, name_cap, "%s", l.name.c_str());
  *count = l.count;
  return SERL_OK;
}

int serl_agent_leaf_layout(serl_agent* a, const char* leaf, int64_t out[5]) {
  SERL_REQUIRE(a && leaf && out, "NULL argument");
  const Leaf* t = find(a->trunk_leaves, leaf);
  const Leaf* l = t ? t : find(a->theta_leaves, leaf);
  SERL_REQUIRE(l != nullptr, "unknown leaf '%s'", leaf);
  if (l->cols == 0) { out[0] = out[1] = out[3] = 1; out[2] = out[4] = l->count; }   // contiguous: one row of count columns
  else { out[0] = l->n; out[1] = l->rows; out[2] = l->cols; out[3] = l->rows_p; out[4] = l->ld; }
  return SERL_OK;
}

static int flush_trunk_ema(serl_agent* a) {
  if (a->trunk_ema_pending > 0 && a->trunk_count > 0) {
    RC(frozen_ema(a->trunk, a->trunk_t, a->trunk_count, a->cfg.tau, a->trunk_ema_pending, nullptr));
    SERL_HIP(hipDeviceSynchronize());
  }
  a->trunk_ema_pending = 0;
  return SERL_OK;
}

// resolves (section, leaf) -> device pointer (nullptr = outside that optimizer's support: exact zeros, as the gradient there)
// *lp: the leaf, whose storage behind *ptr may be a box (param_arena.h)
static int resolve(serl_agent* a, const char* section, const char* leaf, float** ptr, const Leaf** lp) {
  const Leaf* t = find(a->trunk_leaves, leaf);
  const Leaf* l = t ? t : find(a->theta_leaves, leaf);
  SERL_REQUIRE(l != nullptr, "unknown leaf '%s'", leaf);
  *lp = l;
  const std::string s(section);
  const Offs& o = a->o;
  if (s == "params") { *ptr = (t ? a->trunk : a->theta) + l->off; return SERL_OK; }
  if (s == "target_params") { *ptr = (t ? a->trunk_t : a->theta_t) + l->off; return SERL_OK; }
  const bool mu = s.size() > 3 && s.substr(s.size() - 3) == "/mu";
  const bool nu = s.size() > 3 && s.substr(s.size() - 3) == "/nu";
  SERL_REQUIRE(s.rfind("opt/", 0) == 0 && (mu || nu), "unknown section '%s'", section);
  const std::string tx = s.substr(4, s.size() - 7);
  *ptr = nullptr;
  if (t) return SERL_OK;
  if (tx == "critic") {
    if (l->off < o.Pc) *ptr = (mu ? a->m_c : a->v_c) + l->off;
  } else if (tx == "actor") {
    if (l->off >= o.Pa0 && l->off < o.Pa1) *ptr = (mu ? a->m_a : a->v_a) + (l->off - o.Pa0);
  } else if (tx == "temperature") {
    if (l->off == o.lam) *ptr = mu ? a->m_t : a->v_t;
  } else {
    set_error("unknown optimizer '%s'", tx.c_str());
    return SERL_ERR_INVALID;
  }
  return SERL_OK;
}

}  // extern "C"
// ---- the agent as a snapshot handle sees it (internal.h; snapshot.hip) ----
namespace serl {
// (*count: the leaf's STORAGE, padding included -- what a contiguous copy of the leaf has to cover)
int agent_resolve(serl_agent* a, const char* section, const char* leaf, float** ptr, long* count) {
  const Leaf* l;
  RC(resolve(a, section, leaf, ptr, &l));
  *count = l->span();
  return SERL_OK;
}
int agent_device(const serl_agent* a) { return a->cfg.device; }
int64_t agent_trunk_gen(const serl_agent* a) { return a->trunk_gen; }
void agent_snapshot_count(serl_agent* a, int delta) { a->snapshots += delta; }
int agent_flush_target_trunk(serl_agent* a, hipStream_t stream) {
  if (a->trunk_ema_pending > 0 && a->trunk_count > 0) RC(frozen_ema(a->trunk, a->trunk_t, a->trunk_count, a->cfg.tau, a->trunk_ema_pending, stream));
  a->trunk_ema_pending = 0;
  return SERL_OK;
}
}  // namespace serl
extern "C" {

static constexpr const char* kOutsideSupport = "'%s' of '%s' lies outside the optimizer's support and must be zero";

int serl_agent_set(serl_agent* a, const char* section, const char* leaf, const float* host, int64_t count) {
  SERL_REQUIRE(a && section && leaf && host, "NULL argument");
  SERL_HIP(hipSetDevice(a->cfg.device));
  float* p; const Leaf* l;
  RC(resolve(a, section, leaf, &p, &l));
  SERL_REQUIRE(l->count == count, "leaf '%s' has %ld elements, got %lld", leaf, l->count, (long long)count);
  if (std::strncmp(leaf, "trunk/", 6) == 0) { SERL_HIP(hipDeviceSynchronize()); RC(flush_trunk_ema(a)); }   // pending EMA steps belong to the old values
  RC(leaf_copy(p, nullptr, host, *l, hipMemcpyHostToDevice, section, kOutsideSupport));
  if (p && std::strncmp(leaf, "trunk/", 6) == 0) {
    a->tpk.dirty = true;
    if (a->live) { a->tpk_t.dirty = true; a->trunk_ver += 1; a->trunk_t_ver += 1; }   // (either copy: both are re-packed and re-evaluated)
    a->trunk_gen += 1;   // (a reward classifier attached on equal trunks is stale now: check_label_fresh)
  }
  return SERL_OK;
}

int serl_agent_get(serl_agent* a, const char* section, const char* leaf, float* host_out, int64_t count) {
  SERL_REQUIRE(a && section && leaf && host_out, "NULL argument");
  SERL_HIP(hipSetDevice(a->cfg.device));
  float* p; const Leaf* l;
  RC(resolve(a, section, leaf, &p, &l));
  SERL_REQUIRE(l->count == count, "leaf '%s' has %ld elements, got %lld", leaf, l->count, (long long)count);
  if (p) {
    SERL_HIP(hipDeviceSynchronize());
    if (std::strncmp(leaf, "trunk/", 6) == 0 && std::strcmp(section, "target_params") == 0) RC(flush_trunk_ema(a));
  }
  return leaf_copy(p, host_out, nullptr, *l, hipMemcpyDeviceToHost, section, kOutsideSupport);
}

int serl_agent_set_trunk_mode(serl_agent* a, int mode) {
  SERL_REQUIRE(a && (mode == 0 || mode == 1), "trunk mode must be 0 (fp32) or 1 (f16x3)");
  a->trunk_mode = mode;
  return SERL_OK;
}

int serl_agent_set_chain_budget(serl_agent* a, int workgroups) {
  SERL_REQUIRE(a && workgroups >= 0 && workgroups <= 8192, "bad K-split budget");
  a->split_budget = workgroups;
  return SERL_OK;
}

int serl_agent_set_step(serl_agent* a, int64_t step) {
  SERL_REQUIRE(a && step >= 0, "bad argument");
  a->step = step;
  return SERL_OK;
}
int64_t serl_agent_get_step(serl_agent* a) { return a ? a->step : -1; }

int serl_agent_trunk_forward(serl_agent* a, const uint8_t* dev_frames, int n, float* dev_feats_out, void* stream) {
  SERL_REQUIRE(a && dev_frames && dev_feats_out, "NULL argument");
  SERL_REQUIRE(!a->state_only && !a->small, "this agent has no frozen trunk");
  SERL_HIP(hipSetDevice(a->cfg.device));
  return trunk_forward(a->tw, a->tws, dev_frames, n, dev_feats_out, (hipStream_t)stream, a->trunk_mode ? &a->tpk : nullptr);
}

static int check_batch(serl_agent* a, const serl_batch* b) {
  const serl_agent_cfg& c = a->cfg;
  // (an agent without the proprio branch never reads the state: NULL is accepted)
  SERL_REQUIRE(b && (b->frames || c.n_cam == 0) && (b->state || a->opts.no_proprio) && b->action && b->reward && b->mask, "serl_batch has NULL members");
  SERL_REQUIRE(b->batch >= 1 && b->batch <= c.batch, "batch %d not in [1,%d]", b->batch, c.batch);
  SERL_REQUIRE(b->n_cam == c.n_cam && (c.n_cam == 0 || (b->H == c.H && b->W == c.W && b->C == 3)) &&
                   b->state_dim == c.state_dim && b->act_dim == c.act_dim, "serl_batch shape does not match the agent");
  SERL_REQUIRE((b->num_stack > 0 ? b->num_stack : 1) == c.num_stack, "serl_batch.num_stack %d does not match the agent's num_stack %d",
               b->num_stack > 0 ? b->num_stack : 1, c.num_stack);
  return SERL_OK;
}

static int trunk_pass(serl_agent* a, const serl_batch* batch, float* feats, int stage_begin, int stage_end, hipStream_t st);

int serl_agent_encode_slot(serl_agent* a, const serl_batch* batch, int slot, void* stream) {
  return serl_agent_encode_slot_range(a, batch, slot, -1, kTrunkStages - 1, stream);
}

int serl_agent_encode_slot_range(serl_agent* a, const serl_batch* batch, int slot, int stage_begin, int stage_end, void* stream) {
  SERL_REQUIRE(a, "NULL agent");
  SERL_REQUIRE(slot >= 0 && slot < serl_agent::kSlots, "slot must be 0..%d", serl_agent::kSlots - 1);
  SERL_REQUIRE(stage_begin >= -1 && stage_begin <= stage_end && stage_end < kTrunkStages, "bad stage range [%d, %d]", stage_begin, stage_end);
  int rc = check_batch(a, batch);
  if (rc) return rc;
  SERL_HIP(hipSetDevice(a->cfg.device));
  hipStream_t st = (hipStream_t)stream;
  a->cur_slot[slot] = *batch;
  a->slot_valid[slot] = true;
  if (a->live) return SERL_OK;   // the phases compute their features themselves, behind the apply in front of them (live_features)
  return trunk_pass(a, batch, a->feats_slot[slot], stage_begin, stage_end, st);
}

// The frozen trunk on both observation sides of `batch` into `feats` ([2][n_cam][cfg.batch] feature maps)
static int trunk_pass(serl_agent* a, const serl_batch* batch, float* feats, int stage_begin, int stage_end, hipStream_t st) {
  const serl_agent_cfg& c = a->cfg;
  const int B = batch->batch;
  const size_t fbytes = (size_t)c.H * c.W * 3;
  if (a->state_only || a->small) return SERL_OK;  // no frozen encoder: nothing to precompute
  if (B == c.batch) {  // frames [2][n_cam][B] are one contiguous run of 2*n_cam*B images
    // (sub-batching the run to keep activations in the Infinity Cache was measured: slower -- DESIGN.md)
    return trunk_forward(a->tw, a->tws, batch->frames, 2 * c.n_cam * B, feats, st, a->trunk_mode ? &a->tpk : nullptr, stage_begin, stage_end);
  }
  SERL_REQUIRE(stage_begin < 0 && stage_end == kTrunkStages - 1, "partial trunk passes need a full-size batch");
  for (int w = 0; w < 2; ++w)
    for (int k = 0; k < c.n_cam; ++k)
      RC(trunk_forward(a->tw, a->tws, batch->frames + ((size_t)(w * c.n_cam + k) * B) * fbytes, B,
                       feats + (((long)w * c.n_cam + k) * c.batch) * a->HW * 512, st, a->trunk_mode ? &a->tpk : nullptr));
  return SERL_OK;
}

// Live trunk.  Rows [off, off + cnt) of the sides [w0, w1) of `batch` (0 = observations, 1 = next observations) through the trunk
// copy (w, pk) into `feats`, laid out [w1 - w0][n_cam][cfg.batch] feature maps: the whole run of images in one pass where it is
// contiguous on both ends, else one pass per (side, camera) as in trunk_pass.
static int trunk_rows(serl_agent* a, const TrunkWeights& w, TrunkPacked& pk, const serl_batch* batch, int w0, int w1, int off, int cnt,
                      float* feats, hipStream_t st) {
  const serl_agent_cfg& c = a->cfg;
  const int B = batch->batch;
  const size_t fbytes = (size_t)c.H * c.W * 3;
  const long fmap = (long)a->HW * 512;
  SERL_REQUIRE(off >= 0 && cnt >= 1 && off + cnt <= B && B <= c.batch, "trunk rows [%d, %d) outside a batch of %d", off, off + cnt, B);
  TrunkPacked* packed = a->trunk_mode ? &pk : nullptr;
  if (off == 0 && cnt == B && B == c.batch)
    return trunk_forward(w, a->tws, batch->frames + (size_t)w0 * c.n_cam * B * fbytes, (w1 - w0) * c.n_cam * B, feats, st, packed);
  for (int s = w0; s < w1; ++s)
    for (int k = 0; k < c.n_cam; ++k)
      RC(trunk_forward(w, a->tws, batch->frames + ((size_t)(s * c.n_cam + k) * B + off) * fbytes, cnt,
                       feats + (((long)(s - w0) * c.n_cam + k) * c.batch + off) * fmap, st, packed));
  return SERL_OK;
}

// Live trunk: what the phase about to run on rows [off, off + cnt) of the selected batch reads -- both sides through the online
// trunk and, with `target`, the next frames through the target copy (sac.py:143-147 with target_params) -- is computed here, on the
// phase's stream and therefore behind every apply enqueued so far, unless the slot already holds it for the current version of
// that copy.  update_high_utd thus runs a pass per minibatch (each apply moved the trunk) and one over the whole batch in front of
// its actor phase; update() with all three networks runs one, shared by its phases.
static int live_features(serl_agent* a, int off, int cnt, bool target, hipStream_t st) {
  if (!a->live) return SERL_OK;
  auto stale = [&](const serl_agent::FeatRows& h, int64_t ver) { return h.ver != ver || off < h.lo || off + cnt > h.hi; };
  if (stale(a->feats_on, a->trunk_ver)) {
    RC(trunk_rows(a, a->tw, a->tpk, &a->cur, 0, 2, off, cnt, a->feats, st));
    a->feats_on.ver = a->trunk_ver; a->feats_on.lo = off; a->feats_on.hi = off + cnt;
  }
  if (target && stale(a->feats_tg, a->trunk_t_ver)) {
    RC(trunk_rows(a, a->tw_t, a->tpk_t, &a->cur, 1, 2, off, cnt, a->feats_t, st));
    a->feats_tg.ver = a->trunk_t_ver; a->feats_tg.lo = off; a->feats_tg.hi = off + cnt;
  }
  return SERL_OK;
}

static constexpr const char* kLiveNoRemote =
    "this agent's trunk is live (weight decay on the pretrained trunk): features computed elsewhere would be those of another trunk";

int serl_agent_slot_features(serl_agent* a, int slot, float** dev_out, int64_t* count_out) {
  SERL_REQUIRE(a && dev_out && count_out, "NULL argument");
  SERL_REQUIRE(slot >= 0 && slot < serl_agent::kSlots, "slot must be 0..%d", serl_agent::kSlots - 1);
  SERL_REQUIRE(!a->state_only && !a->small, "this agent has no frozen-trunk features");
  if (a->live) { set_error("%s", kLiveNoRemote); return SERL_ERR_UNSUPPORTED; }
  *dev_out = a->feats_slot[slot];
  *count_out = 2LL * a->cfg.n_cam * a->cfg.batch * a->HW * 512;
  return SERL_OK;
}

int serl_agent_bind_slot(serl_agent* a, const serl_batch* batch, int slot) {
  SERL_REQUIRE(a, "NULL agent");
  SERL_REQUIRE(slot >= 0 && slot < serl_agent::kSlots, "slot must be 0..%d", serl_agent::kSlots - 1);
  int rc = check_batch(a, batch);
  if (rc) return rc;
  SERL_REQUIRE(batch->batch == a->cfg.batch, "externally computed features cover a full-size batch");
  if (a->live) { set_error("%s", kLiveNoRemote); return SERL_ERR_UNSUPPORTED; }
  a->cur_slot[slot] = *batch;
  a->slot_valid[slot] = true;
  return SERL_OK;
}

int serl_agent_select_slot(serl_agent* a, int slot) {
  SERL_REQUIRE(a, "NULL agent");
  SERL_REQUIRE(slot >= 0 && slot < serl_agent::kSlots && a->slot_valid[slot], "slot %d holds no encoded batch", slot);
  a->feats = a->feats_slot[slot];
  a->feats_t = a->feats_t_slot[slot];
  a->feats_on = a->feats_tg = serl_agent::FeatRows{};   // (live trunk: nothing of this batch is computed yet)
  a->cur = a->cur_slot[slot];
  a->has_batch = true;
  a->labelled = a->label_exempt = false;   // this batch's rewards are its own until serl_agent_label_rewards runs
  return SERL_OK;
}

int serl_agent_encode(serl_agent* a, const serl_batch* batch, void* stream) {
  RC(serl_agent_encode_slot(a, batch, 0, stream));
  return serl_agent_select_slot(a, 0);
}

int serl_agent_begin_update(serl_agent* a, void* stream) {
  SERL_REQUIRE(a, "NULL agent");
  SERL_HIP(hipSetDevice(a->cfg.device));
  (void)stream;
  a->info_reset = true;  // the next critic step's info kernel zeroes the accumulators (no memset launch)
  return SERL_OK;
}

// mlp.py:27-28; sac.py:137-176,197-207: the Dropout draws of the next update / phase / dry-run call (serl_mi355.h)
int serl_agent_set_mlp_noise(serl_agent* a, const serl_mlp_noise* noise) {
  SERL_REQUIRE(a, "NULL agent");
  SERL_REQUIRE(a->mlp_depth == 0, "serl_agent_set_mlp_noise inside an update");
  a->mlp_bound = noise ? *noise : serl_mlp_noise{};
  return SERL_OK;
}

int serl_agent_set_shard(serl_agent* a, int64_t global_offset, int64_t global_batch) {
  SERL_REQUIRE(a, "NULL agent");
  SERL_REQUIRE(global_batch == 0 || (global_offset >= 0 && global_offset < global_batch), "bad shard [%lld of %lld]",
               (long long)global_offset, (long long)global_batch);
  a->shard_off = global_batch ? global_offset : 0;
  a->shard_global = global_batch;
  return SERL_OK;
}

// ---- reward labelling (vice.py:546,594) -----------------------------------------------------------------------------------
// A trunk leaf set on either handle since the attach may have made the trunks differ: the shared-feature path would then label
// from features the classifier's own trunk does not produce.  Refused until the caller attaches again (which compares anew).
static int check_label_fresh(serl_agent* a) {
  if (!a->cls) return SERL_OK;
  const bool mine = a->trunk_gen != a->attach_gen, theirs = classifier_view(a->cls).trunk_gen != a->attach_cls_gen;
  if (mine || theirs) {
    set_error("stale reward-classifier attachment: a trunk leaf of the %s was set after serl_agent_set_reward_classifier; attach again",
              mine ? "agent" : "classifier");
    return SERL_ERR_STATE;
  }
  return SERL_OK;
}

int serl_agent_set_reward_classifier(serl_agent* a, serl_classifier* cls, const int* cam_of, int* mode_out) {
  SERL_REQUIRE(a, "NULL agent");
  if (!cls) {
    a->cls = nullptr;
    a->label_mode = SERL_LABEL_NONE;
    a->labelled = false;
    if (mode_out) *mode_out = SERL_LABEL_NONE;
    return SERL_OK;
  }
  SERL_REQUIRE(cam_of, "NULL camera map");
  const serl_agent_cfg& c = a->cfg;
  SERL_REQUIRE(!a->state_only, "a state-only agent has no frames for a reward classifier to label");
  SERL_REQUIRE(c.num_stack == 1, "the reward classifier reads single frames (its pretrained conv_init takes 3 channels): an agent with num_stack %d "
               "cannot be labelled by it", c.num_stack);
  const ClassifierView v = classifier_view(cls);
  SERL_REQUIRE(v.cfg.device == c.device, "the classifier lives on device %d, the agent on %d", v.cfg.device, c.device);
  for (int k = 0; k < v.cfg.n_cam; ++k)
    SERL_REQUIRE(cam_of[k] >= 0 && cam_of[k] < c.n_cam, "classifier camera %d maps to agent camera %d, the agent has %d", k, cam_of[k], c.n_cam);
  SERL_REQUIRE(v.cfg.H == c.H && v.cfg.W == c.W, "the classifier takes %dx%d images, the agent %dx%d", v.cfg.H, v.cfg.W, c.H, c.W);
  SERL_REQUIRE(v.cfg.max_batch >= c.batch, "classifier max_batch %d is below the agent's batch %d", v.cfg.max_batch, c.batch);
  SERL_HIP(hipSetDevice(c.device));
  int mode = SERL_LABEL_FRAMES;
  // (a live trunk is the classifier's only until the first optimizer step: always the classifier's own pass)
  if (!a->small && !a->live && v.trunk_count == a->trunk_count) {   // shared features only where every trunk leaf is bit-identical
    SERL_HIP(hipDeviceSynchronize());
    std::vector<float> mine(a->trunk_count), theirs(a->trunk_count);
    SERL_HIP(hipMemcpy(mine.data(), a->trunk, sizeof(float) * mine.size(), hipMemcpyDeviceToHost));
    SERL_HIP(hipMemcpy(theirs.data(), v.trunk, sizeof(float) * theirs.size(), hipMemcpyDeviceToHost));
    if (std::memcmp(mine.data(), theirs.data(), sizeof(float) * mine.size()) == 0) mode = SERL_LABEL_FEATURES;
  }
  a->cls = cls;
  for (int k = 0; k < v.cfg.n_cam; ++k) a->cls_cam[k] = cam_of[k];
  a->label_mode = mode;
  a->attach_gen = a->trunk_gen;
  a->attach_cls_gen = v.trunk_gen;
  a->labelled = false;
  if (mode_out) *mode_out = mode;
  return SERL_OK;
}

int serl_agent_label_rewards(serl_agent* a, void* stream) {
  SERL_REQUIRE(a && a->has_batch, "serl_agent_encode / serl_agent_select_slot must run first");
  if (!a->cls) {
    set_error("no reward classifier is attached (serl_agent_set_reward_classifier)");
    return SERL_ERR_STATE;
  }
  RC(check_label_fresh(a));
  const serl_agent_cfg& c = a->cfg;
  hipStream_t st = (hipStream_t)stream;
  SERL_HIP(hipSetDevice(c.device));
  const int n = a->cur.batch, nc = classifier_view(a->cls).cfg.n_cam;
  SERL_HIP(hipMemsetAsync(a->label_ctr, 0, sizeof(int), st));
  if (a->label_mode == SERL_LABEL_FEATURES) {   // pass 1 of the slot: the augmented next observations, camera stride = cfg.batch maps
    const long cam_stride = (long)c.batch * a->HW * 512;
    RC(classifier_label(a->cls, a->feats + c.n_cam * cam_stride, cam_stride, a->cls_cam, nullptr, n, a->labels, a->label_logits,
                        a->label_mean, a->label_ctr, st));
  } else {
    const size_t fbytes = (size_t)c.H * c.W * 3;
    const uint8_t* cams[SERL_MAX_CAMS];
    for (int k = 0; k < nc; ++k) cams[k] = a->cur.frames + ((size_t)(c.n_cam + a->cls_cam[k]) * n) * fbytes;   // frames[1][camera]
    RC(classifier_label(a->cls, nullptr, 0, nullptr, cams, n, a->labels, a->label_logits, a->label_mean, a->label_ctr, st));
  }
  a->label_n = n;
  a->labelled = true;
  return SERL_OK;
}

int serl_agent_reward_label_rows(serl_agent* a) { return a ? a->label_n : -1; }

int serl_agent_read_reward_labels(serl_agent* a, float* host_labels, float* host_logits, float* mean_out, void* stream) {
  SERL_REQUIRE(a, "NULL agent");
  SERL_REQUIRE(a->label_n > 0, "no rewards were labelled yet");
  hipStream_t st = (hipStream_t)stream;
  SERL_HIP(hipSetDevice(a->cfg.device));
  const size_t bytes = sizeof(float) * a->label_n;
  if (host_labels) SERL_HIP(hipMemcpyAsync(host_labels, a->labels, bytes, hipMemcpyDeviceToHost, st));
  if (host_logits) SERL_HIP(hipMemcpyAsync(host_logits, a->label_logits, bytes, hipMemcpyDeviceToHost, st));
  if (mean_out) SERL_HIP(hipMemcpyAsync(mean_out, a->label_mean, sizeof(float), hipMemcpyDeviceToHost, st));
  SERL_HIP(hipStreamSynchronize(st));
  return SERL_OK;
}

int serl_agent_critic_grads(serl_agent* a, int off, int cnt, int global_count, const serl_noise* noise,
                            int redq_row, void* stream) {
  return serl_agent_critic_grads_bucketed(a, off, cnt, global_count, noise, redq_row, stream, nullptr);
}

int serl_agent_grad_bucket(serl_agent* a, int bucket, float** dev_ptr, int64_t* count) {
  SERL_REQUIRE(a && dev_ptr && count, "NULL argument");
  SERL_REQUIRE(bucket == 0 || bucket == 1, "bucket must be 0 or 1");
  const Offs& o = a->o;
  if (bucket == 0) { *dev_ptr = a->Gc + o.c[0].W; *count = (o.Pc - o.c[0].W) + kScalars; }
  else { *dev_ptr = a->Gc; *count = o.c[0].W; }
  return SERL_OK;
}

int serl_agent_critic_grads_bucketed(serl_agent* a, int off, int cnt, int global_count, const serl_noise* noise,
                                     int redq_row, void* stream, void* event_bucket0) {
  MlpNoiseScope mlp_scope(a);
  SERL_REQUIRE(a && a->has_batch, "serl_agent_encode must run first");
  SERL_REQUIRE(off >= 0 && cnt >= 1 && off + cnt <= a->cur.batch && global_count >= cnt, "bad minibatch range");
  RC(mlp_masks_fit(a));
  if (a->cls && !a->labelled && !a->label_exempt) {
    set_error("a reward classifier is attached: serl_agent_label_rewards must follow serl_agent_select_slot (vice.py:594)");
    return SERL_ERR_STATE;
  }
  const serl_agent_cfg& c = a->cfg;
  const Offs& o = a->o;
  hipStream_t st = (hipStream_t)stream;
  SERL_HIP(hipSetDevice(c.device));
  // REDQ subsample (sac.py:150-157): critic_subsample_size members drawn with replacement; cfg 0 = the launcher's 2,
  // -1 = None (the minimum runs over the whole ensemble and nothing is drawn)
  const int m_sub = c.critic_subsample_size == 0 ? 2 : (c.critic_subsample_size < 0 ? 0 : c.critic_subsample_size);
  SERL_REQUIRE(m_sub <= 16, "critic_subsample_size %d exceeds 16", m_sub);
  RedqSel sel{};
  sel.n = m_sub;
  if (noise && noise->redq_idx) {
    for (int k = 0; k < m_sub; ++k) sel.idx[k] = noise->redq_idx[m_sub * redq_row + k];
  } else {  // randint(0, ensemble) with replacement
    uint64_t r = c.seed * 0x9E3779B97F4A7C15ull + (++a->noise_ctr) * 0xBF58476D1CE4E5B9ull;
    for (int k = 0; k < m_sub; ++k) {
      r ^= r >> 29; r *= 0x94D049BB133111EBull; r ^= r >> 32;
      sel.idx[k] = (int)(r % c.ensemble);
      r += 0x9E3779B97F4A7C15ull;
    }
  }
  for (int k = 0; k < m_sub; ++k) SERL_REQUIRE(sel.idx[k] >= 0 && sel.idx[k] < c.ensemble, "REDQ index out of range");
  a->pg_ncs = a->pg_nwg = 0;
  a->pg_defer = true;
  const int A = c.act_dim;
  PhaseNoise nz = draw_noise(a, noise ? noise->eps_next : nullptr, noise ? noise->mask_next : nullptr, 0,
                             noise && noise->key_eps_next ? noise->key_eps_next + 2 * redq_row : nullptr,
                             noise && noise->key_mask_next ? noise->key_mask_next + 2 * c.n_cam * redq_row : nullptr);
  RC(materialise_noise(a, &nz, 1, off, cnt, global_count, st));
  RC(live_features(a, off, cnt, true, st));
  // the three encoder passes of the critic loss in one set of launches: online policy input at next_obs
  // (dropout), target-critic input at next_obs (target_params, train=False), online-critic input at obs
  // (train=False; the batch's actions ride along into [enc | action])
  EncJob ej[3] = {{a->theta, 1, nullptr, &a->encP, nullptr, nullptr},
                  {a->theta_t, 1, nullptr, &a->encT, nullptr, nullptr},
                  {a->theta, 0, nullptr, &a->encO, a->cur.action + (long)off * A, a->crit.x + a->E}};
  if (a->live) ej[1].x = a->feats_t;   // target_params hold the target trunk too
  // backup_entropy (sac.py:174-176) needs alpha = softplus(lagrange) of the online parameters next to the per-sample log-probs
  PolJob pj{a->theta, &a->pol, a->encP.enc, a->encP.ld, nullptr, a->critT.x + a->E, a->XA, nullptr,
            c.backup_entropy ? a->aux + X_ALPHA : nullptr};
  set_noise(a, ej[0], pj, nz, off, cnt, global_count);
  // the MLPs' Dropout in the reference's draw order (sac.py:137-176): policy at next_obs, target critic, online critic
  CritJob cj[2] = {{a->theta_t, &a->critT, {}}, {a->theta, &a->crit, {}}};  // target and online ensembles together
  mlp_sites(a, SERL_SITE_PI_NEXT, a->opts.policy.dropout, off, cnt, global_count, redq_row, pj.drop);
  mlp_sites(a, SERL_SITE_Q_TARGET, a->opts.critic.dropout, off, cnt, global_count, redq_row, cj[0].drop);
  mlp_sites(a, SERL_SITE_Q_ONLINE, a->opts.critic.dropout, off, cnt, global_count, redq_row, cj[1].drop);
  RC(encode_multi(a, ej, 3, off, cnt, st));
  RC(policy_fwd_multi(a, &pj, 1, cnt, st));
  RC(critic_fwd_multi(a, cj, 2, cnt, st));
  const float* reward = a->labelled ? a->labels : a->cur.reward;   // vice.py:594: the labels stand in for the stored rewards
  const LossArgs L{1, a->critT.q, a->crit.q, reward + off, a->cur.mask + off, sel, c.ensemble, cnt, c.discount,
                   1.0f / ((float)c.ensemble * (float)global_count), a->ytgt, a->dq, a->SC, a->Gc + o.c_hb, a->state_only ? 1 : 0,
                   c.backup_entropy ? a->pol.logp : nullptr, c.backup_entropy ? a->aux + X_ALPHA : nullptr};
  SERL_REQUIRE(!a->state_only || c.ensemble <= 16, "per-member head bias supports ensembles of at most 16");
  RC(critic_bwd(a, a->theta, a->crit, cnt, true, st, &L, 0.f, cj[1].drop));
  RC(enc_bwd_critic(a, a->theta, a->encO, off, cnt, st, event_bucket0));
  RC(flush_param_grads(a, st));
  a->last_global = global_count;
  return SERL_OK;
}

int serl_agent_actor_grads(serl_agent* a, int global_count, const serl_noise* noise, void* stream) {
  MlpNoiseScope mlp_scope(a);
  SERL_REQUIRE(a && a->has_batch, "serl_agent_encode must run first");
  const serl_agent_cfg& c = a->cfg;
  const Offs& o = a->o;
  hipStream_t st = (hipStream_t)stream;
  SERL_HIP(hipSetDevice(c.device));
  const int cnt = a->cur.batch, A = c.act_dim, top = o.na - 1, Hd = o.a[top].N;   // the head reads the policy's last layer
  SERL_REQUIRE(global_count >= cnt, "global_count < local batch");
  RC(mlp_masks_fit(a));
  a->pg_ncs = a->pg_nwg = 0;
  a->pg_defer = true;
  enum { PI = 0, TEMP = 1 };   // noise of the policy loss (slot 1) and of the temperature loss (slot 2), drawn in this order
  PhaseNoise nz[2] = {draw_noise(a, noise ? noise->eps_pi : nullptr, noise ? noise->mask_obs_pi : nullptr, 1,
                                 noise ? noise->key_eps_pi : nullptr, noise ? noise->key_mask_obs_pi : nullptr),
                      draw_noise(a, noise ? noise->eps_temp : nullptr, noise ? noise->mask_next_temp : nullptr, 2,
                                 noise ? noise->key_eps_temp : nullptr, noise ? noise->key_mask_next_temp : nullptr)};
  RC(materialise_noise(a, nz, 2, 0, cnt, global_count, st));
  RC(live_features(a, 0, cnt, false, st));
  // encoder passes of the actor step in one set of launches: temperature loss input (next_obs, dropout;
  // sac.py:223-234), critic-side encoding of obs (train=False), policy input at obs (dropout; sac.py:193-221)
  EncJob ej[3] = {{a->theta, 1, nullptr, &a->encT, nullptr, nullptr},
                  {a->theta, 0, nullptr, &a->encO, nullptr, nullptr},
                  {a->theta, 0, nullptr, &a->encP, nullptr, nullptr}};
  PolJob pj[2] = {{a->theta, &a->polT, a->encT.enc, a->encT.ld, nullptr, a->act_tmp, A, a->SC + S_LOGP_NEXT, a->aux + X_ALPHA},
                  {a->theta, &a->pol, a->encP.enc, a->encP.ld, nullptr, a->crit.x + a->E, a->XA, a->SC + S_LOGP, nullptr}};
  set_noise(a, ej[0], pj[0], nz[TEMP], 0, cnt, global_count);
  set_noise(a, ej[2], pj[1], nz[PI], 0, cnt, global_count);
  // the MLPs' Dropout (sac.py:197-207,222-227): policy at obs, the critic inside the actor loss, policy at next_obs
  CritJob cj{a->theta, &a->crit, {}};
  mlp_sites(a, SERL_SITE_PI, a->opts.policy.dropout, 0, cnt, global_count, 0, pj[1].drop);
  mlp_sites(a, SERL_SITE_Q_ACTOR, a->opts.critic.dropout, 0, cnt, global_count, 0, cj.drop);
  mlp_sites(a, SERL_SITE_PI_TEMP, a->opts.policy.dropout, 0, cnt, global_count, 0, pj[0].drop);
  RC(encode_multi(a, ej, 3, 0, cnt, st));
  RC(policy_fwd_multi(a, pj, 2, cnt, st));
  const float* eps_pi = nz[PI].eps ? nz[PI].eps : nz[PI].eps_out;   // (the backward reads the draws the head used)
  RC(critic_fwd_multi(a, &cj, 1, cnt, st));
  RC(critic_bwd(a, a->theta, a->crit, cnt, false, st, nullptr, -1.0f / ((float)c.ensemble * (float)global_count), cj.drop));
  RC(policy_dist_bwd(a->dx + a->E, a->XA, a->crit.x + a->E, a->XA, a->pol.pre, a->pol.std, eps_pi, a->aux + X_ALPHA,
                     1.0f / (float)global_count, cnt, A, c.std_min, c.std_max, a->dpre, a->crit.q, c.ensemble,
                     a->SC + S_QPI, st, a->pol_mode));
  // policy heads (mean, log_std): two groups with uniform stride; parameter gradients off the critical chain.  kPolUniform: one
  // group, and hs = A is the distance from the mean's bias to log_stds.  kPolFixed: one group and no std leaf -- dpre is the
  // mean's slab alone, so neither the second group's weight gradient nor the log_stds column sum exists
  const long hs = head_stride(a);
  const int hg = a->head_groups;
  float* Ga = a->Ga - o.Pa0;   // Ga[o] = gradient of the actor-tx leaf at parameter offset o
  const float* P = a->theta;
  const MlpBuf& pm = a->pol.m;
  const auto io = [&](int l) { return l ? mlp_io(o.a[l], pm.l[l - 1], pm.l[l], cnt) : mlp_io(o.a[0], a->encP.enc, a->encP.ld, pm.l[0], cnt); };
  const DenseLnGrad dtop = mlp_grad(o.a[top], a->s[top], cnt), d1 = mlp_grad(o.a[0], a->s[0], cnt);
  // (the head is no Dense -> LayerNorm layer -- no LayerNorm, mean and log_std as groups: its three GEMM forms are written out)
  RC(wgrad(a, gemm_wgrad(pm.l[top].h, Hd, 0, a->dpre, A, (long)cnt * A, Ga + o.a_Wm, A, hs, hg, Hd, A, cnt), st));
  RC(head_bias_grad(a, cnt, Ga + o.a_bm, hs, st));
  // dh = dmean W_mean^T + dlog_std W_logstd^T (no second term when the log-std has no Dense)
  RC(igrad_sum(a, gemm_igrad(a->dpre, A, (long)cnt * A, P + o.a_Wm, A, hs, nullptr, 0, 0, hg, cnt, Hd, A), dtop.dy, dtop.ld_dy, st));
  for (int l = top; l >= 0; --l) {
    const DenseLnGrad d = mlp_grad(o.a[l], a->s[l], cnt);
    RC(dense_ln_bwd(a, o.a[l], P, io(l), d, cnt, Ga, st, nullptr, pj[1].drop[l]));
    if (l) RC(gemm_f32(layer_igrad(o.a[l], P, d, cnt, mlp_grad(o.a[l - 1], a->s[l - 1], cnt)), st));
  }
  // image codes are stop-gradiented (encoding.py:48-49); only the proprio slice of d_enc is needed: the rows of W1 that the
  // proprio columns multiply, a slice of layer 1's kernel and therefore written out
  if (a->prop) {   // (an image-only policy has no trainable input: its backward ends at layer 1)
    const DenseLnGrad dp{a->sprop.dy, o.prop.N, 0, a->sprop.dpre, a->sprop.dg};
    RC(gemm_f32(gemm_igrad(d1.dpre, o.a[0].N, 0, P + o.a[0].W + (long)c.n_cam * o.cam.N * o.a[0].N, o.a[0].N, 0, dp.dy, dp.ld_dy, 0, 1, cnt,
                           o.prop.N, o.a[0].N), st));
    RC(dense_ln_bwd(a, o.prop, P, prop_io(a, a->encP, a->cur.state), dp, cnt, Ga, st));
  }
  RC(flush_param_grads(a, st));
  a->last_global = global_count;
  return SERL_OK;
}

int serl_agent_apply(serl_agent* a, int which, float info_weight, void* stream) {
  SERL_REQUIRE(a, "NULL agent");
  SERL_REQUIRE(which >= 1 && which <= 7, "bad `which` (a non-empty set of SERL_NET_* bits)");
  const serl_agent_cfg& c = a->cfg;
  const Offs& o = a->o;
  hipStream_t st = (hipStream_t)stream;
  SERL_HIP(hipSetDevice(c.device));
  const bool crit = which & SERL_NET_CRITIC, act = which & SERL_NET_ACTOR, temp = which & SERL_NET_TEMPERATURE;
  AdamArgs ad{};
  ad.theta = a->theta; ad.theta_target = a->theta_t;
  ad.P = o.P; ad.Pc = o.Pc; ad.Pa0 = o.Pa0; ad.Pa1 = o.Pa1;
  ad.g_critic = a->Gc; ad.g_actor = a->Ga;
  ad.m_c = a->m_c; ad.v_c = a->v_c; ad.m_a = a->m_a; ad.v_a = a->v_a; ad.m_t = a->m_t; ad.v_t = a->v_t;
  ad.sum_logp_next = a->SC + S_LOGP_NEXT; ad.temp_grad_out = a->aux + X_TGRAD;
  ad.critic_on = crit ? 1 : 0; ad.actor_on = act ? 1 : 0; ad.temp_on = temp ? 1 : 0;
  ad.ema_on = crit ? 1 : 0;   // sac.py:284-285
  // all three txs share count == step (common.py:136-168 steps every optimizer on every update)
  ad.lr_a = lr_at(c, a->step, SERL_TX_ACTOR);
  ad.lr_c = lr_at(c, a->step, SERL_TX_CRITIC);
  ad.lr_t = lr_at(c, a->step, SERL_TX_TEMPERATURE);
  const int64_t t = a->step + 1;
  ad.bc1 = 1.0f - powf(0.9f, (float)t);
  ad.bc2 = 1.0f - powf(0.999f, (float)t);
  ad.tau = c.tau; ad.target_entropy = c.target_entropy;
  ad.inv_batch = a->last_global > 0 ? 1.0f / (float)a->last_global : 0.f;
  ad.frozen = a->trunk; ad.frozen_target = a->trunk_t; ad.n_frozen = a->trunk_count;  // common.py:124-134 covers every leaf
  if (!a->live && a->trunk_count > 0) {   // frozen leaves only ever see the EMA: count the step, apply it lazily (flush_trunk_ema)
    ad.n_frozen = 0;
    if (crit) a->trunk_ema_pending += 1;
  }
  ad.wd_a = c.tx_weight_decay_on[SERL_TX_ACTOR] ? c.tx_weight_decay[SERL_TX_ACTOR] : 0.f;
  ad.wd_c = c.tx_weight_decay_on[SERL_TX_CRITIC] ? c.tx_weight_decay[SERL_TX_CRITIC] : 0.f;
  ad.wd_t = c.tx_weight_decay_on[SERL_TX_TEMPERATURE] ? c.tx_weight_decay[SERL_TX_TEMPERATURE] : 0.f;
  ad.clip_a = c.tx_clip_norm[SERL_TX_ACTOR]; ad.clip_c = c.tx_clip_norm[SERL_TX_CRITIC]; ad.clip_t = c.tx_clip_norm[SERL_TX_TEMPERATURE];
  ad.norm2 = a->aux + X_NORM2;
  if ((ad.clip_c > 0.f && crit) || (ad.clip_a > 0.f && act))
    RC(grad_norm2(a->Gc, o.Pc, a->Ga, o.Pa1 - o.Pa0, a->aux + X_NORM2, st));
  ad.info_mode = (crit ? 1 : 0) | ((act || temp) ? 2 : 0);
  ad.info_reset = (crit && a->info_reset) ? 1 : 0;
  if (crit) a->info_reset = false;
  ad.scalars = a->SC; ad.alpha = a->aux + X_ALPHA; ad.info_acc = a->info_acc;
  ad.info_w = info_weight;
  ad.inv_eb = a->last_global > 0 ? 1.0f / ((float)c.ensemble * (float)a->last_global) : 0.f;
  RC(adam_ema(ad, st));
  if (a->live) {   // the step decayed the online trunk and, with the EMA, moved the target copy: planes and features are stale
    a->tpk.dirty = true; a->trunk_ver += 1;
    if (crit) { a->tpk_t.dirty = true; a->trunk_t_ver += 1; }
  }
  a->step += 1;
  a->lr_last[SERL_TX_ACTOR] = ad.lr_a; a->lr_last[SERL_TX_CRITIC] = ad.lr_c; a->lr_last[SERL_TX_TEMPERATURE] = ad.lr_t;
  return SERL_OK;
}

int serl_agent_grad_view(serl_agent* a, int which, float** dev_ptr, int64_t* count) {
  SERL_REQUIRE(a && dev_ptr && count, "NULL argument");
  SERL_REQUIRE(which >= 1 && which <= 7, "bad `which`");
  const Offs& o = a->o;
  const bool crit = which & SERL_NET_CRITIC, at = which & (SERL_NET_ACTOR | SERL_NET_TEMPERATURE);
  if (crit && at) { *dev_ptr = a->G; *count = o.Pc + kScalars + (o.Pa1 - o.Pa0); }
  else if (crit) { *dev_ptr = a->Gc; *count = o.Pc + kScalars; }
  else { *dev_ptr = a->SC; *count = kScalars + (o.Pa1 - o.Pa0); }
  return SERL_OK;
}

int serl_agent_update(serl_agent* a, const serl_batch* batch, int nets, const serl_noise* noise, void* stream) {
  MlpNoiseScope mlp_scope(a);
  SERL_REQUIRE(a && batch, "NULL argument");
  SERL_REQUIRE(nets >= 1 && nets <= 7, "Invalid gradient steps: %d", nets);   // sac.py:272-274
  RC(serl_agent_begin_update(a, stream));
  RC(serl_agent_encode(a, batch, stream));
  a->label_exempt = true;   // SACAgent.update keeps the stored rewards: VICE overrides update_critics / update_high_utd only
  if (nets & SERL_NET_CRITIC) RC(serl_agent_critic_grads(a, 0, batch->batch, batch->batch, noise, 0, stream));
  if (nets & (SERL_NET_ACTOR | SERL_NET_TEMPERATURE)) RC(serl_agent_actor_grads(a, batch->batch, noise, stream));
  return serl_agent_apply(a, nets, 1.0f, stream);
}

int serl_agent_update_critics(serl_agent* a, const serl_batch* batch, const serl_noise* noise, void* stream) {
  MlpNoiseScope mlp_scope(a);
  SERL_REQUIRE(a, "NULL agent");
  RC(check_label_fresh(a));
  RC(serl_agent_begin_update(a, stream));
  RC(serl_agent_encode(a, batch, stream));
  if (a->cls) RC(serl_agent_label_rewards(a, stream));
  RC(serl_agent_critic_grads(a, 0, batch->batch, batch->batch, noise, 0, stream));
  return serl_agent_apply(a, SERL_APPLY_CRITIC, 1.0f, stream);
}

int serl_agent_update_high_utd(serl_agent* a, const serl_batch* batch, int utd_ratio, const serl_noise* noise,
                               void* stream) {
  MlpNoiseScope mlp_scope(a);
  SERL_REQUIRE(a && batch, "NULL argument");
  SERL_REQUIRE(utd_ratio >= 1 && batch->batch % utd_ratio == 0,
               "Batch size %d must be divisible by UTD ratio %d", batch->batch, utd_ratio);  // sac.py:561-563
  RC(check_label_fresh(a));
  RC(serl_agent_begin_update(a, stream));
  RC(serl_agent_encode(a, batch, stream));
  if (a->cls) RC(serl_agent_label_rewards(a, stream));   // once, over the whole batch, before the first minibatch (vice.py:594)
  const int mb = batch->batch / utd_ratio;
  for (int i = 0; i < utd_ratio; ++i) {
    RC(serl_agent_critic_grads(a, i * mb, mb, mb, noise, i, stream));
    RC(serl_agent_apply(a, SERL_APPLY_CRITIC, 1.0f / (float)utd_ratio, stream));
  }
  RC(serl_agent_actor_grads(a, batch->batch, noise, stream));
  return serl_agent_apply(a, SERL_APPLY_ACTOR_TEMP, 1.0f, stream);
}

int serl_agent_read_info(serl_agent* a, serl_info* out, void* stream) {
  SERL_REQUIRE(a && out, "NULL argument");
  SERL_HIP(hipSetDevice(a->cfg.device));
  float acc[I_N];
  SERL_HIP(hipMemcpyAsync(acc, a->info_acc, sizeof(acc), hipMemcpyDeviceToHost, (hipStream_t)stream));
  SERL_HIP(hipStreamSynchronize((hipStream_t)stream));
  out->critic_loss = acc[I_CL]; out->predicted_qs = acc[I_PQ]; out->target_qs = acc[I_TQ];
  out->actor_loss = acc[I_AL]; out->temperature = acc[I_TEMP]; out->entropy = acc[I_ENT];
  out->temperature_loss = acc[I_TL];
  out->actor_lr = a->lr_last[SERL_TX_ACTOR]; out->critic_lr = a->lr_last[SERL_TX_CRITIC];
  out->temperature_lr = a->lr_last[SERL_TX_TEMPERATURE];
  return SERL_OK;
}

// ---- acting and read-only evaluation (serl_mi355.h): forwards on observations that are no update batch ---------------------------
// What the forward helpers read of the agent's host-side training state is swapped for the evaluation's own view and put back
// when the scope ends, on every path out: the batch binding, the feature slot, the reward-label flags, the loss normaliser and
// the noise counter.  Device memory: the evaluations write activations, gradient scratch, the scratch feature slot and eval_info
// only -- nothing a later update reads before it has rewritten it.
struct EvalScope {
  serl_agent* a;
  serl_batch cur; bool has_batch, labelled, label_exempt; float* feats; int last_global; uint64_t noise_ctr;
  float* feats_t; serl_agent::FeatRows feats_on, feats_tg;   // live trunk: the scratch slot starts empty, the update's slot keeps what it holds
  explicit EvalScope(serl_agent* a_)
      : a(a_), cur(a_->cur), has_batch(a_->has_batch), labelled(a_->labelled), label_exempt(a_->label_exempt), feats(a_->feats),
        last_global(a_->last_global), noise_ctr(a_->noise_ctr), feats_t(a_->feats_t), feats_on(a_->feats_on), feats_tg(a_->feats_tg) {
    a->feats = a->feats_slot[serl_agent::kSlots];
    a->feats_t = a->feats_t_slot[serl_agent::kSlots];
    a->feats_on = a->feats_tg = serl_agent::FeatRows{};
  }
  ~EvalScope() {
    a->cur = cur; a->has_batch = has_batch; a->labelled = labelled; a->label_exempt = label_exempt; a->feats = feats;
    a->last_global = last_global; a->noise_ctr = noise_ctr;
    a->feats_t = feats_t; a->feats_on = feats_on; a->feats_tg = feats_tg;
    a->pg_ncs = a->pg_nwg = 0;
  }
};

static int eval_check(serl_agent* a, const uint8_t* dev_frames, const float* dev_state, int n) {
  SERL_REQUIRE(a, "NULL agent");
  const serl_agent_cfg& c = a->cfg;
  SERL_REQUIRE(n >= 1 && n <= c.batch, "n %d not in [1,%d]", n, c.batch);
  SERL_REQUIRE(dev_frames || c.n_cam == 0, "dev_frames is NULL on an agent with %d camera(s)", c.n_cam);
  SERL_REQUIRE(dev_state || a->opts.no_proprio, "dev_state is NULL");
  return SERL_OK;
}

// The trunk on [n_cam][n] images into the scratch slot, then one EncodingWrapper pass with parameters P, train=False (no Dropout),
// into `e`; the state goes through a temporary serl_batch view (with `act_src` the actions ride into [enc | action] at act_dst).
// Inside an EvalScope.
static int eval_encode(serl_agent* a, const uint8_t* dev_frames, const float* dev_state, int n, const float* P, EncBuf* e,
                       const float* act_src, float* act_dst, hipStream_t st) {
  const serl_agent_cfg& c = a->cfg;
  const size_t fbytes = (size_t)c.H * c.W * 3;
  // (live trunk: target_params hold their own trunk copy -- forward_target_critic runs it)
  const bool tgt = a->live && P == a->theta_t;
  const TrunkWeights& w = tgt ? a->tw_t : a->tw;
  TrunkPacked& pk = tgt ? a->tpk_t : a->tpk;
  for (int k = 0; k < c.n_cam && !a->small; ++k)
    RC(trunk_forward(w, a->tws, dev_frames + (size_t)k * n * fbytes, n, a->feats + ((long)k * c.batch) * a->HW * 512, st,
                     a->trunk_mode ? &pk : nullptr));
  a->cur = serl_batch{};
  a->cur.batch = n;
  a->cur.state = const_cast<float*>(dev_state);
  a->cur.frames = const_cast<uint8_t*>(dev_frames);   // (the SmallEncoder reads the pixels in encode_multi)
  const EncJob ej{P, 0, nullptr, e, act_src, act_dst};
  return encode_multi(a, &ej, 1, 0, n, st);
}

int serl_agent_sample_actions(serl_agent* a, const uint8_t* dev_frames, const float* dev_state, int n,
                              const float* dev_eps, float* dev_out_actions, void* stream) {
  SERL_REQUIRE(a && (dev_state || a->opts.no_proprio) && dev_out_actions, "NULL argument");
  const serl_agent_cfg& c = a->cfg;
  SERL_REQUIRE(dev_frames || c.n_cam == 0, "NULL frames");
  SERL_REQUIRE(n >= 1 && n <= c.batch, "n %d not in [1,%d]", n, c.batch);
  hipStream_t st = (hipStream_t)stream;
  SERL_HIP(hipSetDevice(c.device));
  EvalScope scope(a);
  RC(eval_encode(a, dev_frames, dev_state, n, a->theta, &a->encP, nullptr, nullptr, st));
  if (!dev_eps) {  // argmax -> mode = tanh(mean), or the mean itself without the squash: zero noise
    RC(fill(a->eps_buf[0], 0.f, (long)n * c.act_dim, st));
    dev_eps = a->eps_buf[0];
  }
  PolJob pj{a->theta, &a->pol, a->encP.enc, a->encP.ld, dev_eps, dev_out_actions, c.act_dim, nullptr, nullptr};
  pj.eps_out = a->eps_buf[0];
  return policy_fwd_multi(a, &pj, 1, n, st);
}

int serl_agent_eval_q(serl_agent* a, const uint8_t* dev_frames, const float* dev_state, const float* dev_actions,
                      int n, int target, float* dev_q_out, void* stream) {
  RC(eval_check(a, dev_frames, dev_state, n));
  SERL_REQUIRE(dev_actions && dev_q_out, "dev_actions or dev_q_out is NULL");
  const serl_agent_cfg& c = a->cfg;
  hipStream_t st = (hipStream_t)stream;
  SERL_HIP(hipSetDevice(c.device));
  EvalScope scope(a);
  // the target copy goes through the target buffers of the critic phase, the online one through the online buffers
  const float* P = target ? a->theta_t : a->theta;
  CritBuf& cb = target ? a->critT : a->crit;
  RC(eval_encode(a, dev_frames, dev_state, n, P, target ? &a->encT : &a->encO, dev_actions, cb.x + a->E, st));
  const CritJob cj{P, &cb, {}};   // train=False: no Dropout
  RC(critic_fwd_multi(a, &cj, 1, n, st));
  SERL_HIP(hipMemcpyAsync(dev_q_out, cb.q, sizeof(float) * c.ensemble * n, hipMemcpyDeviceToDevice, st));   // [ensemble][n]
  return SERL_OK;
}

int serl_agent_eval_policy(serl_agent* a, const uint8_t* dev_frames, const float* dev_state, const float* dev_actions,
                           int n, float* dev_mean_out, float* dev_std_out, float* dev_mode_out, float* dev_logp_out,
                           void* stream) {
  RC(eval_check(a, dev_frames, dev_state, n));
  SERL_REQUIRE(!dev_logp_out || dev_actions, "dev_logp_out is given and dev_actions is NULL: a log-density needs the actions");
  const serl_agent_cfg& c = a->cfg;
  const Offs& o = a->o;
  hipStream_t st = (hipStream_t)stream;
  SERL_HIP(hipSetDevice(c.device));
  EvalScope scope(a);
  const float* P = a->theta;
  RC(eval_encode(a, dev_frames, dev_state, n, P, &a->encP, nullptr, nullptr, st));
  // the policy MLP as policy_fwd_multi runs it; the head always as a plain K-split GEMM whose slabs policy_stats_kernel reads
  // (whatever a->fuse says: the fused epilogue samples, and this call draws nothing)
  PolBuf& pb = a->pol;
  PolJob pj{};   // train=False: no Dropout site
  pj.P = P; pj.pb = &pb; pj.enc = a->encP.enc; pj.ld_enc = a->encP.ld;
  RC(policy_mlp_multi(a, &pj, 1, n, st));
  const int Hd = o.a[o.na - 1].N;
  const GemmDesc g = gemm_fwd(pb.m.l[o.na - 1].h, Hd, 0, P + o.a_Wm, head_stride(a), a->slabs_lane[0], a->head_groups, n, c.act_dim,
                              Hd, 4);
  SERL_REQUIRE((long)a->head_groups * 4 * n * c.act_dim <= a->slabs_cap, "policy head exceeds the slab scratch");
  RC(gemm_f32_multi(&g, 1, st));
  PolicyStatsArgs v{};
  v.slabs = a->slabs_lane[0]; v.S = 4; v.bias_mean = P + o.a_bm; v.bias_ls = head_bias_ls(a, P); v.act = dev_actions;
  v.mean = dev_mean_out; v.std = dev_std_out; v.mode_out = dev_mode_out; v.logp = dev_logp_out;
  v.rows = n; v.A = c.act_dim; v.std_min = c.std_min; v.std_max = c.std_max; v.mode = a->pol_mode;
  return policy_stats(v, st);
}

int serl_agent_eval_losses(serl_agent* a, const serl_batch* batch, const serl_noise* noise, serl_info* host_out, void* stream) {
  MlpNoiseScope mlp_scope(a);
  SERL_REQUIRE(a && batch && host_out, "NULL argument");
  RC(check_batch(a, batch));
  const serl_agent_cfg& c = a->cfg;
  hipStream_t st = (hipStream_t)stream;
  SERL_HIP(hipSetDevice(c.device));
  EvalScope scope(a);
  // serl_agent_update's encode without a slot: both sides of the batch through the trunk into the scratch slot, no binding
  if (!a->live) RC(trunk_pass(a, batch, a->feats, -1, kTrunkStages - 1, st));   // (live trunk: the phases below compute theirs)
  a->cur = *batch;
  a->has_batch = true;
  a->labelled = false; a->label_exempt = true;   // SACAgent.update keeps the stored rewards
  RC(serl_agent_critic_grads(a, 0, batch->batch, batch->batch, noise, 0, stream));
  RC(serl_agent_actor_grads(a, batch->batch, noise, stream));
  // the info rider of serl_agent_apply(all three networks) with its arguments, alone
  AdamArgs ad{};
  ad.info_mode = 3; ad.info_reset = 1;
  ad.scalars = a->SC; ad.alpha = a->aux + X_ALPHA; ad.info_acc = a->eval_info;
  ad.info_w = 1.0f;
  ad.target_entropy = c.target_entropy;
  ad.inv_batch = a->last_global > 0 ? 1.0f / (float)a->last_global : 0.f;
  ad.inv_eb = a->last_global > 0 ? 1.0f / ((float)c.ensemble * (float)a->last_global) : 0.f;
  RC(adam_info_only(ad, st));
  float acc[I_N];
  SERL_HIP(hipMemcpyAsync(acc, a->eval_info, sizeof(acc), hipMemcpyDeviceToHost, st));
  SERL_HIP(hipStreamSynchronize(st));
  host_out->critic_loss = acc[I_CL]; host_out->predicted_qs = acc[I_PQ]; host_out->target_qs = acc[I_TQ];
  host_out->actor_loss = acc[I_AL]; host_out->temperature = acc[I_TEMP]; host_out->entropy = acc[I_ENT];
  host_out->temperature_loss = acc[I_TL];
  host_out->actor_lr = lr_at(c, a->step, SERL_TX_ACTOR); host_out->critic_lr = lr_at(c, a->step, SERL_TX_CRITIC);
  host_out->temperature_lr = lr_at(c, a->step, SERL_TX_TEMPERATURE);
  return SERL_OK;
}

int64_t serl_debug_chain_launches(void) { return (int64_t)g_chain_launches; }

int serl_agent_trunk_plan(serl_agent* a, char* out, int cap) {
  SERL_REQUIRE(a && out && cap > 0, "bad argument");
  const TrunkPlan& p = a->tws.plan;
  std::string s = "images=" + std::to_string(p.images) + " pool=" + std::to_string(p.pool) + " raw_b0=" + std::to_string(p.raw_b0);
  static const char* kNames[3] = {"conv0", "conv1", "proj"};
  for (int i = 0; i < kTrunkStages; ++i)
    for (int k = 0; k < 3; ++k) {
      const TrunkPlan::L& l = p.conv[i][k];
      if (!l.kern) continue;
      s += " b" + std::to_string(i) + "_" + kNames[k] + "=" + std::string(1, l.kern) + "/" + std::to_string(l.cfg) + "/" +
           std::to_string(l.pmode) + "/f" + std::to_string(l.fused) + "/p" + std::to_string(l.pad) + "x" + std::to_string(l.padw);
    }
  SERL_REQUIRE((int)s.size() < cap, "the plan text takes %d bytes, the buffer holds %d", (int)s.size() + 1, cap);
  snprintf(out, cap, "%s", s.c_str());
  return SERL_OK;
}

int serl_agent_debug_get(serl_agent* a, const char* what, float* host_out, int64_t count) {
  SERL_REQUIRE(a && what && host_out, "NULL argument");
  SERL_HIP(hipSetDevice(a->cfg.device));
  const Offs& o = a->o;
  const std::string w(what);
  const float* p = nullptr;
  long n = 0;
  const serl_agent_cfg& c = a->cfg;
  if (w == "ctr_nonzero") {
    // The last-arriver epilogues (heads.hip) rest on ONE invariant across launches: every arrival counter is zero when a launch
    // starts (the workgroup that draws the last ticket re-zeroes it with a memory-side store).  A lost arrival, a double ticket or a
    // late re-zero leaves a counter non-zero for the NEXT launch, which then never (or twice) reduces a tile.  host_out[0] = the
    // number of non-zero counters after a device synchronise: 0 at every quiescent point (the stress tests assert it).
    SERL_REQUIRE(count == 1, "tap 'ctr_nonzero' holds one value");
    SERL_HIP(hipDeviceSynchronize());
    std::vector<int> h((size_t)kCtrPerLane * kCtrLanes);
    SERL_HIP(hipMemcpy(h.data(), a->ctr, sizeof(int) * h.size(), hipMemcpyDeviceToHost));
    long nz = 0;
    for (int v : h) nz += v != 0;
    host_out[0] = (float)nz;
    return SERL_OK;
  }
  if (w == "small_plan") {
    // The launch plan of the SmallEncoder's last backward pass, kept on the host: [row chunks of layer 0's weight gradient, K-split
    // of the weight-gradient GEMM of layers 1, 2, 3], as launched; zeros before the first backward pass.
    SERL_REQUIRE(a->small, "tap 'small_plan' belongs to the SmallEncoder");
    SERL_REQUIRE(count == kSmallLayers, "tap 'small_plan' holds %d values", kSmallLayers);
    for (int l = 0; l < kSmallLayers; ++l) host_out[l] = (float)a->sws.last_plan[l];
    return SERL_OK;
  }
  if (w == "pad_max_abs") {
    // The invariant of the ragged layout: every float of a box leaf's storage outside its box is exactly 0 in
    // the parameters, the target parameters, both Adam moments of the critic's and the actor's optimizer and both gradient
    // buffers.  host_out[0] = the largest |value| found there after a device synchronise (NaN counts as infinity); 0 without a box.
    SERL_REQUIRE(count == 1, "tap 'pad_max_abs' holds one value");
    SERL_HIP(hipDeviceSynchronize());
    float worst = 0.f;
    std::vector<float> h;
    const auto scan = [&](const float* dev, long lo, long hi) -> int {   // dev[i - lo] holds parameter index i of [lo, hi)
      h.resize((size_t)(hi - lo));
      if (hi > lo) SERL_HIP(hipMemcpy(h.data(), dev, sizeof(float) * h.size(), hipMemcpyDeviceToHost));
      for (const Leaf& l : a->theta_leaves) {
        if (l.cols == 0 || l.span() == l.count || l.off < lo || l.off >= hi) continue;   // (any padding at all, pad ROWS of a one-block leaf included)
        for (long i = 0; i < l.n; ++i)
          for (long r = 0; r < l.rows_p; ++r)
            for (long cc = (r < l.rows ? l.cols : 0); cc < l.ld; ++cc) {
              const float v = std::fabs(h[(size_t)(l.off - lo + (i * l.rows_p + r) * l.ld + cc)]);
              worst = std::isnan(v) ? INFINITY : std::max(worst, v);
            }
      }
      return SERL_OK;
    };
    RC(scan(a->theta, 0, o.P)); RC(scan(a->theta_t, 0, o.P));
    RC(scan(a->m_c, 0, o.Pc)); RC(scan(a->v_c, 0, o.Pc)); RC(scan(a->Gc, 0, o.Pc));
    RC(scan(a->m_a, o.Pa0, o.Pa1)); RC(scan(a->v_a, o.Pa0, o.Pa1)); RC(scan(a->Ga, o.Pa0, o.Pa1));
    host_out[0] = worst;
    return SERL_OK;
  }
  if (w == "g_critic") { p = a->Gc; n = o.Pc; }
  else if (w == "g_actor") { p = a->Ga; n = o.Pa1 - o.Pa0; }
  else if (w == "scalars") { p = a->SC; n = kScalars; }
  else if (w == "q") { p = a->crit.q; n = (long)c.ensemble * c.batch; }
  else if (w == "q_target") { p = a->critT.q; n = (long)c.ensemble * c.batch; }
  else if (w == "target_q") { p = a->ytgt; n = c.batch; }
  else if (w == "x") { p = a->crit.x; n = (long)c.batch * a->XA; }
  else if (w == "x_target") { p = a->critT.x; n = (long)c.batch * a->XA; }
  else if (w == "feats") { p = a->feats; n = 2L * c.n_cam * c.batch * a->HW * 512; }
  else if (w == "logp") { p = a->pol.logp; n = c.batch; }
  else if (w == "std") { p = a->pol.std; n = (long)c.batch * c.act_dim; }   // clipped std [rows][A] of the last policy evaluation in `pol`
  else if (w == "dx") { p = a->dx; n = (long)c.batch * a->XA; }
  // the MLP rows as the last phase left them: the normalised LayerNorm input of layer l = 1.. of an MLP buffer ([rows][that
  // layer's width], the critics' rows member-major), and the gradient wrt the Dense output of the layer-l backward that ran last
  // (the critic's layer l or the policy's: the scratch holds the larger of the two)
  else if (w.rfind("mlp_xhat/", 0) == 0 && w.size() == 16 && w[15] >= '1' && w[15] < '1' + kL) {
    const std::string buf = w.substr(9, 5);
    const MlpBuf* m = buf == "pol__" ? &a->pol.m : buf == "polT_" ? &a->polT.m : buf == "crit_" ? &a->crit.m : buf == "critT" ? &a->critT.m : nullptr;
    const int l = w[15] - '1';
    const serl_mlp_opts& net = buf[0] == 'c' ? a->opts.critic : a->opts.policy;
    if (!m || l >= net.n_layers) { set_error("unknown debug tap '%s'", what); return SERL_ERR_INVALID; }
    p = m->l[l].xhat;
    n = (long)(buf[0] == 'c' ? c.ensemble : 1) * c.batch * net.dims[l];
  }
  else if (w.rfind("mlp_dpre/", 0) == 0 && w.size() == 10 && w[9] >= '1' && w[9] - '1' < std::max(a->opts.critic.n_layers, a->opts.policy.n_layers)) {
    const serl_mlp_opts &critic = a->opts.critic, &policy = a->opts.policy;
    const int l = w[9] - '1';
    p = a->s[l].dpre;
    n = std::max<long>(l < critic.n_layers ? (long)c.ensemble * c.batch * critic.dims[l] : 0, l < policy.n_layers ? (long)c.batch * policy.dims[l] : 0);
  }
  // SmallEncoder layer l's ReLU output of the LAST encoder pass, [n_cam][images of that pass][h_{l+1}][w_{l+1}][cout_l]
  else if (w.rfind("small_act", 0) == 0 && w.size() == 10 && w[9] >= '0' && w[9] < '0' + kSmallLayers && a->small) {
    const int l = w[9] - '0';
    p = a->sws.act[l];
    n = (long)c.n_cam * c.batch * a->sws.d.h[l + 1] * a->sws.d.w[l + 1] * kSmallFeat[l + 1];
  }
  else { set_error("unknown debug tap '%s'", what); return SERL_ERR_INVALID; }
  SERL_REQUIRE(count <= n && count > 0, "tap '%s' holds %ld floats, asked for %lld", what, n, (long long)count);
  SERL_HIP(hipDeviceSynchronize());
  SERL_HIP(hipMemcpy(host_out, p, sizeof(float) * count, hipMemcpyDeviceToHost));
  return SERL_OK;
}

int serl_agent_debug_set(serl_agent* a, const char* what, const float* host, int64_t count) {
  SERL_REQUIRE(a && what && host, "NULL argument");
  SERL_HIP(hipSetDevice(a->cfg.device));
  const Offs& o = a->o;
  const std::string w(what);
  float* p = nullptr;
  long n = 0;
  if (w == "g_critic") { p = a->Gc; n = o.Pc; }
  else if (w == "g_actor") { p = a->Ga; n = o.Pa1 - o.Pa0; }
  else if (w == "scalars") { p = a->SC; n = kScalars; }
  else { set_error("unknown debug tap '%s'", what); return SERL_ERR_INVALID; }
  SERL_REQUIRE(count <= n && count > 0, "tap '%s' holds %ld floats, got %lld", what, n, (long long)count);
  SERL_HIP(hipDeviceSynchronize());
  SERL_HIP(hipMemcpy(p, host, sizeof(float) * count, hipMemcpyHostToDevice));
  if (a->last_global <= 0) a->last_global = 1;
  return SERL_OK;
}

}  // extern "C"
