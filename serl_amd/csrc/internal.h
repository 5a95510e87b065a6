// Internal (non-ABI) interfaces between the translation units of libserl_mi355.so.
#pragma once
#include "common.h"
#include "gn_exchange.h"
#include "param_arena.h"

namespace serl {

// --------------------------------------------------------------------------------------------
// Frozen ResNet-10 trunk (reference: serl_launcher/vision/resnet_v1.py:189-286, config :383-385)
// --------------------------------------------------------------------------------------------
constexpr int kTrunkStages = 4;
constexpr int kStageFilters[kTrunkStages] = {64, 128, 256, 512};
constexpr int kStageStride[kTrunkStages] = {1, 2, 2, 2};
constexpr int kGnGroups = 4;

struct TrunkWeights {  // device pointers into the agent's parameter arena (HWIO conv kernels)
  const float* conv_init;  // [7][7][3][64]
  const float *gn_init_s, *gn_init_b;
  struct Block {
    const float *conv0, *gn0_s, *gn0_b, *conv1, *gn1_s, *gn1_b, *proj, *gnp_s, *gnp_b;
  } blk[kTrunkStages];
};

// Offsets of the trunk's leaves in a flat parameter vector; -1 for the projection of a block that has none.
struct TrunkOffsets {
  long conv_init, gn_init_s, gn_init_b;
  struct Block {
    long conv0, gn0_s, gn0_b, conv1, gn1_s, gn1_b, proj, gnp_s, gnp_b;
  } blk[kTrunkStages];
};
// Appends the trunk's leaves (trunk/conv_init ... trunk/block3/gnp/bias) at `off`, which moves behind them.
TrunkOffsets add_trunk_leaves(std::vector<Leaf>& leaves, long& off);
// The trunk's weights in the parameter vector at `params` (nullptr where the offset is -1).
TrunkWeights trunk_weights(const float* params, const TrunkOffsets& o);

struct TrunkDims {
  int H, W;            // input image
  int h[6], w[6];      // [0]=conv_init out, [1]=pool out, [2..5]=block outputs
};
TrunkDims trunk_dims(int H, int W);

constexpr int kSyncTickets = 16;   // ints per layer; tickets: 8 per launch (one per XCD)
constexpr int kGnLayers = 1 + 3 * kTrunkStages;   // conv_init, then (conv0, conv1, projection) per stage
// Every launch decision of a split-fp16 pass, made by its first piece before anything launches (plan_pass, trunk_f16x3.hip) and
// kept for the pieces that follow; also the introspection of the parity tests (the shapes a data-parallel rank runs choose
// other kernels than the full batch does).
struct TrunkPlan {
  int images = 0;
  bool fuse = false; // the pass uses the fused GroupNorm epilogues (SERL_GN_FUSE and the one-fused-pass-at-a-time claim)
  int pool = 0;      // 0: separate GroupNorm + max-pool pass, 1: pooled in conv_init + pool_finish, 2: completed in conv_init
  int raw_b0 = 0;    // block 0 reads conv_init's raw pooled tensor (RAWIN)
  // kern: 'S' row-slab, 'D' LDS-DMA, 'R' register-staged implicit GEMM, 'F' projection computed by conv0's launch, 0 = layer
  // absent; cfg: tile configuration (9 = the row-slab kernels); pmode: how a wave's rows relate to images (3: statistics by a
  // separate kernel); fused: GroupNorm epilogue inside the conv (1 exchange, 2 local) -- 0 on a conv0 / conv1 means the separate
  // gn_relu_split / block_out pass follows it
  struct L {
    char kern = 0;
    int cfg = 0, pmode = 0, fused = 0;
    int expected = 0, group = 0;   // FuseArgs of a fused launch
    bool raw = false;              // 'S' on conv_init's raw pooled tensor (b0_conv0 of a raw_b0 pass)
    bool proj = false;             // 'D' conv0: the block's projection rides on this launch
    int stagger = 0;               // 'S': ConvArgsB::stagger
    int pad = 0, padw = 0;         // the conv's low-side ("SAME") padding in rows / columns, as conv_geom derived it
  } conv[kTrunkStages][3];
};
struct TrunkWorkspace {
  TrunkPlan plan{};
  int max_images = 0;
  TrunkDims d{};
  float* raw_init = nullptr;  // [N][h0][w0][64]
  float* pool = nullptr;      // [N][h1][w1][64]
  struct B {
    float *raw0, *raw1, *rawp, *out, *norm0;
  } blk[kTrunkStages]{};
  double* stats = nullptr;  // 13 GN layers x [N][4][2]
  int* tickets = nullptr;   // directly behind `stats` (zeroed together, every pass): 13 layers x kSyncTickets ints
  size_t stats_sync_bytes = 0;
  // statistics exchange of the fused GroupNorm epilogues (gn_exchange.h): one 256-byte record per tile that can take part, per layer
  // at record rec_off[layer]; never zeroed between passes -- granules carry the pass `epoch` (0: no pass yet, the first one zeroes)
  uint64_t* rec = nullptr;
  size_t rec_bytes = 0;
  size_t rec_off[kGnLayers] = {};
  uint32_t epoch = 0;
  void* base = nullptr;     // single allocation backing everything above
  size_t bytes = 0;
};
size_t trunk_workspace_bytes(int max_images, int H, int W);
// carve `ws` out of caller-provided device memory (at least trunk_workspace_bytes big)
int trunk_workspace_bind(TrunkWorkspace& ws, void* mem, int max_images, int H, int W);
// split-fp16 copies of the 3x3 / 1x1 conv kernels (trunk_f16x3.hip): fp16 [Cout][K] hi and scaled-lo planes
struct TrunkPacked {
  struct W { uint16_t *hi, *lo; float* inv; uint16_t* dma; } blk[kTrunkStages][3]{};  // dma: copy in the piece order of the LDS-DMA / row-slab kernels, or nullptr
   // [stage][conv0, conv1, proj]; inv = per-output-channel 1/scale
  W init{};                                                   // conv_init planes
  const uint8_t* zero = nullptr;                              // 256 zero bytes (source of out-of-image taps for LDS-DMA loads)
  bool dirty = true;
};
size_t trunk_packed_bytes();
int trunk_packed_bind(TrunkPacked& p, void* mem);
// frames: u8 [n][H][W][3] (device) -> feats: f32 [n][h5][w5][512] (device).
// packed == nullptr: exact fp32 MFMA convs; otherwise the split-fp16 (f16x3) convs for the blocks.
// [stage_begin, stage_end] (split-fp16 path only): -1 = conv_init + pool, 0..3 = residual stages
int trunk_forward(const TrunkWeights& w, TrunkWorkspace& ws, const uint8_t* frames, int n,
                  float* feats_out, hipStream_t stream, TrunkPacked* packed = nullptr, int stage_begin = -1,
                  int stage_end = kTrunkStages - 1);

// --------------------------------------------------------------------------------------------
// small dense building blocks (heads.hip)
// --------------------------------------------------------------------------------------------
// rows are grouped (group g = row / rows_per_group) and every group has its own bias/gamma/beta at
// `pstride` floats apart; the pre-activation is bias + sum of S GEMM slabs laid out [g*S + s][local row][D]
// Dropout between the Dense and the LayerNorm of a row (mlp.py:27-28: x = Dense(x); x = Dropout(rate)(x); x = LayerNorm(x)):
// element (local row r of its group, column c) of the Dense output -- bias included -- is kept and scaled by 1 / keep, or set to
// 0, before the row's statistics are taken.  The keep decision is a function of (r, c) alone, so every group (ensemble member) of
// a launch drops the same elements, as the reference's vmapped critic does (ensemblize splits the params stream only).  The
// backward row states the same decision again and applies it to dx.  mode kLnDropNone: no Dropout -- the rows execute what they
// always did (a wave-uniform branch on this field).
enum { kLnDropNone = 0, kLnDropMask = 1, kLnDropKey = 2, kLnDropHash = 3 };
struct LnDrop {
  int mode;
  float keep;            // 1 - rate, in (0, 1]
  const uint8_t* mask;   // kLnDropMask: u8 [rows_per_group][D], 1 = keep
  // kLnDropKey: jax.random.bernoulli(key, keep, (total_rows, D))[row0 + r][c] (jaxrng.h).  kLnDropHash: the low 24 bits of
  // mix64(seed ^ mix64((row0 + r) * D + c)) against keep * 2^24; row0 = the GLOBAL row of local row 0 (serl_agent_set_shard).
  uint32_t key[2]; uint64_t seed;
  long total_rows, row0;
};
struct LnFwdArgs {
  const float* slabs; int S; long slab_stride;
  const float *bias, *gamma, *beta; long pstride;   // gamma == beta == nullptr: a plain row, no LayerNorm (ln_fwd_multi, heads.h)
  int rows, rows_per_group;
  float* y; long ld_y; long y_goff;  // y[local_row*ld_y + group*y_goff + col] (column slices / group blocks)
  float* xhat;           // [rows][D] or nullptr
  float* rstd;           // [rows] or nullptr
  // optional fused row-dot (critic head, actor_critic_nets.py:65-73): dot_out[row] = sum_col y*dot_w + dot_b[0]
  const float* dot_w; const float* dot_b; float* dot_out;
  long dot_gstride, dot_b_gstride;  // 0: one head shared by all groups (DrQ critic); else per-group heads (ensemblized Critic)
  int act;               // kAct*: the row's activation, per instance (one launch may mix them) and uniform over a wave
  int d;                 // 0: every column of the row is live.  Else the row's true width, 1 <= d < D: columns [d, D) are zero padding
                         // (a ragged MLP layer, heads.h); read by the ragged instantiations alone.  (Lies in the hole behind act.)
  LnDrop drop;           // Dropout on the gathered row, in front of the statistics (zero-initialised: none)
};
// The activation behind a LayerNorm row (mlp.py:19-31: `activations`, a callable or the name of one in flax.linen).  tanh: the MLPs
// as utils/launcher.py configures them, and always the encoder heads; ReLU: also the BinaryClassifier (reward_classifier.py:24-26);
// swish = silu: x * sigmoid(x), mlp.py's own default.  The values are serl_mlp_opts' act.
enum { kActTanh = 0, kActRelu = 1, kActSwish = 2, kActCount = 3 };
// The policy distribution of an agent (serl_agent_opts' std_param / no_tanh) as the head kernels take it, a template parameter:
// the std parameterisation in the low bits, kPolNoTanh on top.  kPolExp (0) is the tanh-Gaussian with std = exp(log_std).
// kPolFixed (SERL_STD_FIXED): the head has no std parameter; std = clip(fixed_std) of a constant vector.
enum { kPolExp = 0, kPolSoftplus = 1, kPolUniform = 2, kPolFixed = 3, kPolStdMask = 3, kPolNoTanh = 4 };
// tanh-Gaussian policy head: slabs = raw head GEMM outputs (mean, log_std); biases added here, result kept in `pre`
struct PolicyDistArgs {
  const float* slabs; int S;  // head GEMM output [mean | log_std][S K-splits][B][A]; kPolUniform: [mean] alone, bias_ls = log_stds
                              // kPolFixed: [mean] alone, bias_ls = the agent's fixed_std vector (the std itself, not its log)
  const float* bias_mean; const float* bias_ls; float* pre; const float* eps;
  float* act; long ld_act; float* logp; float* std_out; float* sum_logp;
  const float* lam; float* alpha_out;  // optional rider: alpha_out[0] = softplus(lam[0])
  // fused form only (GemmDesc::epi == kEpiPolicy): eps == nullptr -> N(0,1) draws hashed from (seed, global row, j), kept in eps_out
  float* eps_out; uint64_t seed; long row_offset;
  int B, A; float std_min, std_max; long slab_ld, slab_stride;
  // tf != 0 (and eps == nullptr): the draws are jax.random.normal(tf_key, (tf_rows, A))[tf_row0 + b][j] instead of the hash (jaxrng.h)
  int tf; uint32_t tf_key[2]; long tf_rows, tf_row0;
  int mode;   // kPol*
};

// Epilogues of the update chain's GEMMs ("last-arriver" fusion, heads.hip): a launch boundary between a K-split GEMM and the
// small kernel that consumed its slabs is replaced by an arrival counter per output tile -- every workgroup stores its slab
// tile write-through (sc1), drains, bumps the tile's counter, and the workgroup that draws the last ticket reads the slabs back
// (sc1 loads) IN INDEX ORDER and finishes the layer.  Same summation order as the separate kernels: bit-identical results.
enum { kEpiNone = 0, kEpiReduce = 1, kEpiPolicy = 3 };
struct GemmDesc {
  const float* A;
  const float* B;
  float* C;            // slab base; slab z at C + z*sCz
  int M, N, K;
  long sAm, sAk, sAb;  // element strides of A[m][k] and per-batch offset
  long sBk, sBn, sBb;
  long ldc, sCz;       // row stride of C and slab stride
  int nbatch, splitk;  // grid.z = nbatch*splitk, z = batch*splitk + split
  // GATHER (SmallEncoder implicit GEMM): A is the VIRTUAL im2col matrix col[row][k] of an NHWC activation tensor at A,
  //   col[row][k] = A[gtab[row] + (k / gseg) * gpitch + k % gseg]  for k < gkbias,   col[row][gkbias] = 1 (the bias column),
  // gseg = 3 * cin (one kernel row: contiguous in NHWC), gpitch = wi * cin, gtab[row] = offset of the patch's first element.
  // Forward: sAk == 1 (m = row, k = column; batch b starts at row b * M); weight gradient: sAm == 1 (m = column, k = row;
  // batch b starts at row b * K).  gseg % 16 == 0.  nullptr = ordinary strided operand.
  const int* gtab = nullptr;
  int gseg = 0, gkbias = 0;
  long gpitch = 0;
  int relu = 0;        // C = max(acc, 0) (splitk == 1 only)
  // ---- last-arriver epilogue (see above).  The slabs C are then a PADDED scratch image: ldc % 64 == 0, whole 64x64 tiles.
  int epi = kEpiNone;
  int* ctr = nullptr;        // arrival counters of this GEMM (zero before the launch; the last arriver re-zeroes its counter)
  // kEpiReduce: out[zg][m][n] = sum of the `zred` consecutive slabs z = zg*zred .. (one counter per 64x64 output tile)
  int zred = 1;
  float* out = nullptr; long ld_out = 0, out_gstride = 0;
  // kEpiPolicy: one counter per 64-row tile; the last of its nbatch * splitk workgroups samples the tanh-Gaussian
  PolicyDistArgs pd;
  GemmDesc() : A(nullptr), B(nullptr), C(nullptr), M(0), N(0), K(0), sAm(0), sAk(0), sAb(0), sBk(0), sBn(0), sBb(0), ldc(0), sCz(0),
               nbatch(0), splitk(0), pd{} {}
};
int gemm_f32(const GemmDesc& g, hipStream_t stream);

// --------------------------------------------------------------------------------------------
// the reward classifier as the agent's reward labelling sees it (classifier.hip; vice.py:546,594)
// --------------------------------------------------------------------------------------------
struct ClassifierView {
  serl_classifier_cfg cfg;
  const float* trunk; long trunk_count;   // device: the frozen trunk's leaves, in add_trunk_leaves order
  int64_t trunk_gen;                      // number of trunk leaves set so far
};
ClassifierView classifier_view(const serl_classifier* c);
// label[i] = sigmoid(logit[i]) >= 0.5 of n rows, train=False, and mean[0] = their mean (device f32[n], [n], [1]; ctr: one zeroed
// arrival counter).  cam_frames == nullptr: the head on trunk features that exist -- classifier camera k reads
// feats + cam_of[k] * cam_stride ([n][h*w][512]).  Else the classifier's own trunk first, on cam_frames[k] (u8[n][H][W][3]).
int classifier_label(serl_classifier* c, const float* feats, long cam_stride, const int* cam_of, const uint8_t* const* cam_frames,
                     int n, float* label, float* logit, float* mean, int* ctr, hipStream_t stream);

// --------------------------------------------------------------------------------------------
// the agent as a snapshot handle sees it (agent.hip; snapshot.hip)
// --------------------------------------------------------------------------------------------
// serl_agent_get's resolver: (section, leaf) -> device range; *ptr == nullptr for a moment outside its optimizer's support
int agent_resolve(serl_agent* a, const char* section, const char* leaf, float** ptr, long* count);
int agent_device(const serl_agent* a);
int64_t agent_trunk_gen(const serl_agent* a);
void agent_snapshot_count(serl_agent* a, int delta);   // live snapshot handles: serl_agent_destroy is refused while there are any
// Enqueues the deferred target-EMA steps of the frozen trunk (serl_agent::trunk_ema_pending) on `stream`, without waiting: the
// target trunk a snapshot packs behind it on the same stream is the one serl_agent_get would read.
int agent_flush_target_trunk(serl_agent* a, hipStream_t stream);

}  // namespace serl
