// Reward classifier (serl_launcher/networks/reward_classifier.py:16-113): the frozen ResNet-10 trunk
// (split-fp16 MFMA convs, trunk_f16x3.hip) -> per camera SpatialLearnedEmbeddings -> Dropout -> Dense -> LayerNorm -> tanh
// (vision/resnet_v1.py:81-116,324-376; common/encoding.py:26-72 with use_proprio=False) -> Dense(256) -> Dropout -> LayerNorm ->
// ReLU -> Dense(1).  Inference (load_classifier_func) runs train=False, where both Dropout layers are the identity: the same
// kernels as the agent's encoder heads (heads.hip); the last LayerNorm launch applies ReLU and the Dense(1) row-dot.
// Training (train_reward_classifier.py, bottom of this file) is opt-in on the same handle and parameter arena.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "dense_layer.h"
#include "jaxrng.h"
#include "ln_stats.h"

using namespace serl;

namespace {
constexpr int kHidden = 256, kBottleneck = 256, kSleFeatures = 8, kSleSplit = 8;

// Opt-in training workspace (serl_classifier_train_init): optax.adam's moments and the gradient of the trainable slice
// [t0, n_params) -- every camera head and the classifier head; the frozen trunk has none -- plus the activations of a train
// step over up to max_batch rows.  "Instance" 0 is the train=True forward, instance 1 the train=False forward of the same rows.
struct ClsTrain {
  int max_batch = 0;
  float lr = 0.f;
  void* arena = nullptr;
  AdamSlice opt{};                               // moments, gradient and update count of the trainable slice
  float *info = nullptr;                         // [2]
  TrunkWorkspace tws{};
  float *feats = nullptr;                        // [n_cam][n][HW][512]
  float *f = nullptr;                            // [2][n_cam][n][D]
  float *slabs = nullptr;                        // K-split GEMM slabs of both instances
  float *enc = nullptr;                          // [2][n][E]
  float *xhat = nullptr, *rstd = nullptr;        // camera LayerNorms of instance 0: [n_cam * n][256], [n_cam * n]
  float *logits = nullptr;                       // [2][n]
  float *hxhat = nullptr, *hdg = nullptr, *dz = nullptr, *dw2in = nullptr;   // head rows [n][256]
  float *dlogit = nullptr, *rowloss = nullptr, *rowcorr = nullptr;           // [n]
  float *denc = nullptr, *dzc = nullptr, *dgc = nullptr, *df = nullptr, *sle_part = nullptr;
  int* ctr = nullptr;
  long slabs_cap = 0;
};
}  // namespace

struct serl_classifier {
  serl_classifier_cfg cfg{};
  int HW = 0, D = 0, E = 0;
  std::vector<Leaf> leaves;       // trunk leaves first, then the heads; offsets into `params`
  long n_params = 0;
  TrunkOffsets to{};
  CamHeadOffsets cam{};
  long o_w1 = 0, o_b1 = 0, o_g1 = 0, o_be1 = 0, o_w2 = 0, o_b2 = 0;
  void* arena = nullptr;
  float* params = nullptr;
  TrunkWeights tw{};
  TrunkWorkspace tws{};
  TrunkPacked tpk{};
  float *feats = nullptr, *f = nullptr, *slabs = nullptr, *enc = nullptr, *h = nullptr;
  int split0 = 1, split1 = 1;
  long t0 = 0, nt = 0;          // trainable slice: the camera heads and the classifier head (behind the trunk)
  ClsTrain* tr = nullptr;       // nullptr: inference only
  int64_t trunk_gen = 0;        // bumped by every trunk leaf set: an agent that labels with this classifier notices (agent.hip)
};

namespace {

void layout(serl_classifier* c) {
  const serl_classifier_cfg& g = c->cfg;
  const TrunkDims d = trunk_dims(g.H, g.W);
  c->HW = d.h[5] * d.w[5];
  c->D = 512 * kSleFeatures;
  c->E = kBottleneck * g.n_cam;
  std::vector<Leaf>& L = c->leaves;
  long off = 0;
  c->to = add_trunk_leaves(L, off);
  c->cam = add_cam_head_leaves(L, off, g.n_cam, c->D, kBottleneck, [&](const std::string& p) { add_leaf(L, off, p + "sle", (long)c->HW * 512 * kSleFeatures); });
  c->o_w1 = add_leaf(L, off, "head/dense0/kernel", (long)c->E * kHidden);
  c->o_b1 = add_leaf(L, off, "head/dense0/bias", kHidden);
  c->o_g1 = add_leaf(L, off, "head/ln/scale", kHidden);
  c->o_be1 = add_leaf(L, off, "head/ln/bias", kHidden);
  c->o_w2 = add_leaf(L, off, "head/dense1/kernel", kHidden);
  c->o_b2 = add_leaf(L, off, "head/dense1/bias", 1);
  c->n_params = off;
  c->t0 = c->cam.first;
  c->nt = off - c->t0;
}

size_t carve(serl_classifier* c, uint8_t* base) {
  const serl_classifier_cfg& g = c->cfg;
  Bump b(base);
  const long n = g.max_batch;
  c->params = b.take<float>(c->n_params + 1);   // (+ the slot adam_ema keeps behind a slice: never read here)
  uint8_t* pk = b.take<uint8_t>(trunk_packed_bytes());
  uint8_t* ws = b.take<uint8_t>(trunk_workspace_bytes(g.max_batch, g.H, g.W));
  c->feats = b.take<float>((size_t)g.n_cam * n * c->HW * 512);
  c->f = b.take<float>((size_t)g.n_cam * n * c->D);
  c->slabs = b.take<float>((size_t)32 * g.n_cam * n * kBottleneck);
  c->enc = b.take<float>(n * c->E);
  c->h = b.take<float>(n * kHidden);
  if (base) {
    trunk_packed_bind(c->tpk, pk);
    trunk_workspace_bind(c->tws, ws, g.max_batch, g.H, g.W);
    c->tw = trunk_weights(c->params, c->to);
  }
  return b.off;
}

// The frozen trunk on n frames per camera (camera k: u8[n][H][W][3] at cams[k]) -> c->feats [n_cam][max_batch][HW][512]
int own_trunk(serl_classifier* c, const uint8_t* const* cams, int n, hipStream_t st) {
  const long nmax = c->cfg.max_batch;
  for (int k = 0; k < c->cfg.n_cam; ++k)
    RC(trunk_forward(c->tw, c->tws, cams[k], n, c->feats + (long)k * nmax * c->HW * 512, st, &c->tpk));
  return SERL_OK;
}

// Everything between the trunk and the head's LayerNorm, on trunk features that already exist: camera k reads
// feats + cam_of[k] * cam_stride ([n][HW][512]).  Per camera SpatialLearnedEmbeddings -> Dense(256) (K-split GEMM) -> LayerNorm ->
// tanh, written side by side, then Dense_0 as *S1 K-split slabs [S1][n][256] in c->slabs.
int head_slabs(serl_classifier* c, const float* feats, long cam_stride, const int* cam_of, int n, hipStream_t st, int* S1_out) {
  const serl_classifier_cfg& g = c->cfg;
  SERL_REQUIRE(n >= 1 && n <= g.max_batch, "n = %d not in [1, max_batch = %d]", n, g.max_batch);
  SERL_REQUIRE(cam_stride >= (long)n * c->HW * 512, "camera stride %ld holds fewer than n = %d feature maps", cam_stride, n);
  bool affine = true;   // cam_of[k] = cam_of[0] + k * d: the cameras' features are one (possibly negative) stride apart
  for (int k = 0; k < g.n_cam; ++k) {
    SERL_REQUIRE(cam_of[k] >= 0, "negative camera index");
    if (k >= 2 && cam_of[k] - cam_of[k - 1] != cam_of[1] - cam_of[0]) affine = false;
  }
  const float* P = c->params;
  const long nmax = g.max_batch;
  if (affine) {
    const long d = g.n_cam > 1 ? cam_of[1] - cam_of[0] : 0;
    SleFwdArgs sv{feats + cam_of[0] * cam_stride, P + c->cam.first, nullptr, c->f};
    RC(sle_fwd_multi(&sv, 1, 1.0f, n, c->HW, 512, g.n_cam, d * cam_stride, c->cam.stride, 0, nmax * c->D, st));
  } else {
    for (int k = 0; k < g.n_cam; ++k) {
      SleFwdArgs sv{feats + cam_of[k] * cam_stride, P + c->cam.first + k * c->cam.stride, nullptr, c->f + k * nmax * c->D};
      RC(sle_fwd_multi(&sv, 1, 1.0f, n, c->HW, 512, 1, 0, 0, 0, 0, st));
    }
  }
  const int S0 = split_under(n, kBottleneck, g.n_cam, 32);
  const DenseLnIo tc{c->f, c->D, nmax * c->D, c->enc, c->E, kBottleneck, nullptr, nullptr};
  const GemmDesc g0 = layer_fwd(c->cam.dense, P, tc, n, c->slabs, S0);
  const LnFwdArgs l0 = layer_ln_fwd(c->cam.dense, P, tc, n, g0);
  RC(gemm_f32_multi(&g0, 1, st));
  RC(ln_fwd_multi(&l0, 1, kBottleneck, st));
  const int S1 = split_under(n, kHidden, 1, 8);
  // (Dense_0 feeds a Dropout in front of its LayerNorm when training, so its slabs go to label_rows / cls_head_kernel: written out)
  const GemmDesc g1 = gemm_fwd(c->enc, c->E, 0, P + c->o_w1, 0, c->slabs, 1, n, kHidden, c->E, S1);
  RC(gemm_f32_multi(&g1, 1, st));
  *S1_out = S1;
  return SERL_OK;
}

// The head's last launch on Dense_0's slabs: LayerNorm -> ReLU -> Dense(1), logits to dev_logits
LnFwdArgs head_ln_args(serl_classifier* c, int S1, int n, float* dev_logits) {
  const float* P = c->params;
  LnFwdArgs l1{};
  l1.slabs = c->slabs; l1.S = S1; l1.slab_stride = (long)n * kHidden;
  l1.bias = P + c->o_b1; l1.gamma = P + c->o_g1; l1.beta = P + c->o_be1; l1.pstride = 0;
  l1.rows = n; l1.rows_per_group = n;
  l1.y = c->h; l1.ld_y = kHidden; l1.y_goff = 0;
  l1.act = kActRelu;
  l1.dot_w = P + c->o_w2; l1.dot_b = P + c->o_b2; l1.dot_out = dev_logits;
  return l1;
}

}  // namespace

// ---- the classifier as the agent's reward labeller sees it (internal.h) -------------------------------------------------------
namespace serl {

ClassifierView classifier_view(const serl_classifier* c) {
  return ClassifierView{c->cfg, c->params, c->t0, c->trunk_gen};   // (the trunk's leaves lie in front of the first camera head)
}

int classifier_label(serl_classifier* c, const float* feats, long cam_stride, const int* cam_of, const uint8_t* const* cam_frames,
                     int n, float* label, float* logit, float* mean, int* ctr, hipStream_t st) {
  const serl_classifier_cfg& g = c->cfg;
  SERL_REQUIRE(n >= 1 && n <= g.max_batch, "n = %d not in [1, classifier max_batch = %d]", n, g.max_batch);
  int ident[SERL_MAX_CAMS] = {0, 1, 2, 3};
  if (cam_frames) {   // own-trunk path: the classifier's trunk on the frames, then its features in camera order
    RC(own_trunk(c, cam_frames, n, st));
    feats = c->feats; cam_stride = (long)g.max_batch * c->HW * 512; cam_of = ident;
  }
  int S1 = 0;
  RC(head_slabs(c, feats, cam_stride, cam_of, n, st, &S1));
  return label_rows(head_ln_args(c, S1, n, logit), label, mean, ctr, st);
}

}  // namespace serl

extern "C" {

int serl_classifier_create(const serl_classifier_cfg* cfg, serl_classifier** out) {
  SERL_REQUIRE(cfg && out, "NULL argument");
  SERL_REQUIRE(cfg->n_cam >= 1 && cfg->n_cam <= SERL_MAX_CAMS, "n_cam %d not in [1,%d]", cfg->n_cam, SERL_MAX_CAMS);
  SERL_REQUIRE(cfg->H >= 32 && cfg->W >= 32 && cfg->max_batch >= 1, "bad classifier shape");
  SERL_HIP(hipSetDevice(cfg->device));
  serl_classifier* c = new serl_classifier();
  c->cfg = *cfg;
  layout(c);
  if (int rc = alloc_zeroed(&c->arena, carve(c, nullptr), "classifier arena")) {
    delete c;
    return rc;
  }
  carve(c, (uint8_t*)c->arena);
  *out = c;
  return SERL_OK;
}

int serl_classifier_destroy(serl_classifier* c) {
  if (!c) return SERL_OK;
  if (c->tr) {
    if (c->tr->arena) (void)hipFree(c->tr->arena);
    delete c->tr;
  }
  if (c->arena) (void)hipFree(c->arena);
  delete c;
  return SERL_OK;
}

int serl_classifier_num_leaves(serl_classifier* c) { return c ? (int)c->leaves.size() : 0; }

int serl_classifier_leaf_info(serl_classifier* c, int i, char* name_out, int name_cap, int64_t* count) {
  SERL_REQUIRE(c && i >= 0 && i < (int)c->leaves.size(), "leaf index %d out of range", i);
  const Leaf& l = c->leaves[i];
  if (name_out && name_cap > 0) snprintf(name_out, name_cap, "%s", l.name.c_str());
  if (count) *count = l.count;
  return SERL_OK;
}

int serl_classifier_set(serl_classifier* c, const char* leaf, const float* host, int64_t count) {
  SERL_REQUIRE(c && leaf && host, "NULL argument");
  const Leaf* l = find(c->leaves, leaf);
  SERL_REQUIRE(l, "unknown classifier leaf '%s'", leaf);
  SERL_REQUIRE(count == l->count, "leaf '%s' has %ld elements, got %ld", leaf, l->count, (long)count);
  SERL_HIP(hipSetDevice(c->cfg.device));
  SERL_HIP(hipMemcpy(c->params + l->off, host, (size_t)count * 4, hipMemcpyHostToDevice));
  if (l->name.rfind("trunk/", 0) == 0) {
    c->tpk.dirty = true;   // fp16 planes are re-packed on the next forward
    c->trunk_gen += 1;
  }
  return SERL_OK;
}

int serl_classifier_get(serl_classifier* c, const char* leaf, float* host_out, int64_t count) {
  SERL_REQUIRE(c && leaf && host_out, "NULL argument");
  const Leaf* l = find(c->leaves, leaf);
  SERL_REQUIRE(l, "unknown classifier leaf '%s'", leaf);
  SERL_REQUIRE(count == l->count, "leaf '%s' has %ld elements, got %ld", leaf, l->count, (long)count);
  SERL_HIP(hipSetDevice(c->cfg.device));
  SERL_HIP(hipMemcpy(host_out, c->params + l->off, (size_t)count * 4, hipMemcpyDeviceToHost));
  return SERL_OK;
}

int serl_classifier_logits(serl_classifier* c, const uint8_t* dev_frames, int n, float* dev_logits, void* stream) {
  SERL_REQUIRE(c && dev_frames && dev_logits, "NULL argument");
  const serl_classifier_cfg& g = c->cfg;
  SERL_REQUIRE(n >= 1 && n <= g.max_batch, "n = %d not in [1, max_batch = %d]", n, g.max_batch);
  hipStream_t st = (hipStream_t)stream;
  SERL_HIP(hipSetDevice(g.device));
  const uint8_t* cams[SERL_MAX_CAMS];
  for (int k = 0; k < g.n_cam; ++k) cams[k] = dev_frames + (size_t)k * n * g.H * g.W * 3;
  RC(own_trunk(c, cams, n, st));
  int cam_of[SERL_MAX_CAMS];
  for (int k = 0; k < g.n_cam; ++k) cam_of[k] = k;
  return serl_classifier_logits_from_features(c, c->feats, (int64_t)g.max_batch * c->HW * 512, cam_of, n, dev_logits, stream);
}

int serl_classifier_logits_from_features(serl_classifier* c, const float* dev_feats, int64_t cam_stride_floats, const int* cam_of,
                                         int n, float* dev_logits, void* stream) {
  SERL_REQUIRE(c && dev_feats && cam_of && dev_logits, "NULL argument");
  hipStream_t st = (hipStream_t)stream;
  SERL_HIP(hipSetDevice(c->cfg.device));
  int S1 = 0;
  RC(head_slabs(c, dev_feats, cam_stride_floats, cam_of, n, st, &S1));
  const LnFwdArgs l1 = head_ln_args(c, S1, n, dev_logits);
  return ln_fwd_multi(&l1, 1, kHidden, st);
}

}  // extern "C"

// =============================================================================================
// Training (examples/async_cable_route_drq/train_reward_classifier.py:122-137, the same file in
// async_bin_relocation_fwbw_drq): loss = mean(optax.sigmoid_binary_cross_entropy(logits_train, labels)) with both Dropout(0.1)
// layers active (the camera heads' behind SpatialLearnedEmbeddings, resnet_v1.py:351-352, and the head's between Dense_0 and
// LayerNorm_0, reward_classifier.py:23-24); train_accuracy = mean((sigmoid(logits_eval) >= 0.5) == labels) from a train=False
// forward with the pre-update parameters; optax.adam(1e-4) over every leaf (reward_classifier.py:62-66).  The trunk sits behind
// stop_gradient (resnet_v1.py:285-286): its gradient and moments are zero, so Adam leaves it as it is and only the slice
// [t0, n_params) is stepped.  One frozen-trunk pass serves both forwards.
// =============================================================================================
namespace {

__device__ __forceinline__ float cls_softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// One classifier-head row per wave (lane = four adjacent columns of the 256), instance = blockIdx.y (0: train, 1: eval):
//   x = b1 + sum_s slab[s];  train: x = where(keep, x / 0.9, 0);  LayerNorm -> ReLU -> Dense(1) -> logit
// With labels, the train instance also writes its BCE term, dlogit = (sigmoid(l) - y) / n and the backward through Dense(1),
// ReLU, LayerNorm and the Dropout down to dz (the gradient of Dense_0's output) plus the per-row inputs of the column sums:
// dg (-> d scale = sum dg * xhat, d bias = sum dg), dw2in = dlogit * h (-> dDense_1 kernel); the eval instance writes whether
// sigmoid(l) >= 0.5 matches the label (fp32 sigmoid as jax.nn.sigmoid: a logit just below zero may round to 0.5).
struct ClsHeadArgs {
  const float* slabs; int S; long sstride, istride;   // instance i, split s: slabs + i * istride + s * sstride, [n][256]
  const float *b1, *g1, *be1, *w2, *b2;
  int n; float keep;
  const uint8_t* mask;          // keep-mask u8 [n][256] of the train instance, or nullptr
  int gen; uint32_t key[2];     // mask == nullptr && gen: jax.random.bernoulli(key, keep, (n, 256))
  const float* labels;          // [n], or nullptr (forward only)
  float* logits;                // [instances][n]
  float *xhat, *dg, *dz, *dw2in, *dlogit, *rowloss, *rowcorr;
};
__global__ __launch_bounds__(256) void cls_head_kernel(ClsHeadArgs a) {
  const int inst = blockIdx.y;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.n) return;
  const bool train = inst == 0;
  const float* sl = a.slabs + inst * a.istride + (long)row * kHidden;
  float v[4];
  bool keep[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = lane * 4 + j;
    float x = a.b1[col];
    for (int s = 0; s < a.S; ++s) x += sl[(long)s * a.sstride + col];
    keep[j] = true;
    if (train) {
      const long e = (long)row * kHidden + col;
      keep[j] = a.mask ? a.mask[e] != 0
                       : (a.gen ? bits_to_unit(random_bits_at(a.key[0], a.key[1], (uint64_t)a.n * kHidden, (uint64_t)e)) < a.keep : true);
      x = keep[j] ? x / a.keep : 0.f;
    }
    v[j] = x;
  }
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) { s1 += v[j]; s2 += v[j] * v[j]; }
  wave_sum2(s1, s2);
  float mean, rstd;
  ln_mean_rstd<kHidden>(s1, s2, mean, rstd);
  float xh[4], pre[4], h[4], d = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = lane * 4 + j;
    xh[j] = (v[j] - mean) * rstd;
    pre[j] = xh[j] * a.g1[col] + a.be1[col];
    h[j] = fmaxf(pre[j], 0.f);
    d += h[j] * a.w2[col];
  }
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) d += __shfl_xor(d, off);
  const float logit = d + a.b2[0];
  if (lane == 0) a.logits[(long)inst * a.n + row] = logit;
  if (!a.labels) return;
  const float y = a.labels[row];
  const float p = 1.f / (1.f + expf(-logit));
  if (!train) {
    if (lane == 0) a.rowcorr[row] = ((p >= 0.5f ? 1.f : 0.f) == y) ? 1.f : 0.f;
    return;
  }
  const float dl = (p - y) / (float)a.n;
  if (lane == 0) {   // optax.sigmoid_binary_cross_entropy = -y log_sigmoid(l) - (1 - y) log_sigmoid(-l)
    a.rowloss[row] = y * cls_softplus(-logit) + (1.f - y) * cls_softplus(logit);
    a.dlogit[row] = dl;
  }
  float dA[4], dxh[4];
  s1 = 0.f; s2 = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = lane * 4 + j;
    dA[j] = pre[j] > 0.f ? dl * a.w2[col] : 0.f;
    dxh[j] = dA[j] * a.g1[col];
    s1 += dxh[j];
    s2 += dxh[j] * xh[j];
  }
  wave_sum2(s1, s2);
  const float m1 = s1 * (1.0f / kHidden), m2 = s2 * (1.0f / kHidden);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long e = (long)row * kHidden + lane * 4 + j;
    const float dx = rstd * (dxh[j] - m1 - xh[j] * m2);
    a.dz[e] = keep[j] ? dx / a.keep : 0.f;
    a.xhat[e] = xh[j];
    a.dg[e] = dA[j];
    a.dw2in[e] = dl * h[j];
  }
}

// info[0] = mean of the BCE terms, info[1] = mean of the eval hits: one workgroup, 256 strided partial sums then a halving tree
// (a fixed order: deterministic)
__global__ __launch_bounds__(256) void cls_info_kernel(const float* rowloss, const float* rowcorr, int n, float* info) {
  __shared__ float red[2][256];
  const int tid = threadIdx.x;
  float sl = 0.f, sc = 0.f;
  for (int r = tid; r < n; r += 256) { sl += rowloss[r]; sc += rowcorr[r]; }
  red[0][tid] = sl;
  red[1][tid] = sc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) { red[0][tid] += red[0][tid + o]; red[1][tid] += red[1][tid + o]; }
    __syncthreads();
  }
  if (tid == 0) {
    info[0] = red[0][0] / (float)n;
    info[1] = red[1][0] / (float)n;
  }
}

// Backward of the camera heads' Dropout (resnet_v1.py:352): df[cam][e] = where(keep, df / 0.9, 0) in place, e < n * 4096, the
// keep-mask injected ([n_cam][n][4096]) or re-drawn from the camera's key exactly as the SLE forward drew it
struct ClsDropArgs { float* df; long per_cam; const uint8_t* mask; uint32_t key[SERL_MAX_CAMS][2]; float keep; };
__global__ __launch_bounds__(256) void cls_dropout_bwd_kernel(ClsDropArgs a) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= a.per_cam) return;
  const int cam = blockIdx.y;
  const long i = (long)cam * a.per_cam + e;
  const bool k = a.mask ? a.mask[i] != 0
                        : bits_to_unit(random_bits_at(a.key[cam][0], a.key[cam][1], (uint64_t)a.per_cam, (uint64_t)e)) < a.keep;
  a.df[i] = k ? a.df[i] / a.keep : 0.f;
}

size_t carve_train(serl_classifier* c, ClsTrain* t, uint8_t* base) {
  const serl_classifier_cfg& g = c->cfg;
  Bump b(base);
  const long n = t->max_batch, nc = g.n_cam;
  t->opt.carve(b, c->t0, c->nt);
  t->info = b.take<float>(2);
  uint8_t* ws = b.take<uint8_t>(trunk_workspace_bytes((int)(nc * n), g.H, g.W));
  t->feats = b.take<float>((size_t)nc * n * c->HW * 512);
  t->f = b.take<float>((size_t)2 * nc * n * c->D);
  t->slabs_cap = 2L * 32 * nc * n * kBottleneck;
  t->slabs = b.take<float>(t->slabs_cap);
  t->enc = b.take<float>((size_t)2 * n * c->E);
  t->xhat = b.take<float>((size_t)nc * n * kBottleneck);
  t->rstd = b.take<float>((size_t)nc * n);
  t->logits = b.take<float>((size_t)2 * n);
  t->hxhat = b.take<float>((size_t)n * kHidden);
  t->hdg = b.take<float>((size_t)n * kHidden);
  t->dz = b.take<float>((size_t)n * kHidden);
  t->dw2in = b.take<float>((size_t)n * kHidden);
  t->dlogit = b.take<float>(n);
  t->rowloss = b.take<float>(n);
  t->rowcorr = b.take<float>(n);
  t->denc = b.take<float>((size_t)n * c->E);
  t->dzc = b.take<float>((size_t)nc * n * kBottleneck);
  t->dgc = b.take<float>((size_t)nc * n * kBottleneck);
  t->df = b.take<float>((size_t)nc * n * c->D);
  t->sle_part = b.take<float>((size_t)nc * kSleSplit * c->HW * 512 * kSleFeatures);
  t->ctr = b.take<int>((size_t)nc * c->HW * cdiv(512, 256));
  if (base) trunk_workspace_bind(t->tws, ws, (int)(nc * n), g.H, g.W);
  return b.off;
}

constexpr float kKeep = 0.9f;   // nn.Dropout(0.1): keep probability 1 - 0.1

// The train=True forward (instance 0) and, with `eval`, the train=False forward (instance 1) of n cropped observations up to the
// classifier-head kernel.  masks: u8 [n_cam][n][4096] then [n][256] (device) or nullptr; keys: host uint32 [n_cam + 1][2] -- the
// make_rng("dropout") keys of encoder_def/encoder_<k>/Dropout_0 and of the root Dropout_0.
// the camera layer's tensors of instance i: the train instance alone keeps the statistics its backward reads
DenseLnIo train_cam_io(const serl_classifier* c, int n, int i) {
  const ClsTrain* t = c->tr;
  const long nD = (long)n * c->D;
  return DenseLnIo{t->f + i * c->cfg.n_cam * nD, c->D, nD, t->enc + (long)i * n * c->E, c->E, kBottleneck, i ? nullptr : t->xhat, i ? nullptr : t->rstd};
}

int train_forward(serl_classifier* c, const uint8_t* frames, int n, const float* labels, const uint8_t* masks,
                  const uint32_t* keys, bool eval, hipStream_t st) {
  const serl_classifier_cfg& g = c->cfg;
  ClsTrain* t = c->tr;
  const float* P = c->params;
  const int nc = g.n_cam, ni = eval ? 2 : 1;
  const long nD = (long)n * c->D;
  RC(trunk_forward(c->tw, t->tws, frames, nc * n, t->feats, st, &c->tpk));
  // SpatialLearnedEmbeddings (+ Dropout keep-mask on instance 0) of both instances in one launch
  SleFwdArgs sv[2] = {SleFwdArgs{}, SleFwdArgs{}};
  for (int i = 0; i < ni; ++i) { sv[i].x = t->feats; sv[i].K = P + c->cam.first; sv[i].f = t->f + i * nc * nD; }
  sv[0].mask = masks;
  if (!masks) sle_tf_masks(sv[0], keys, nc, n, 0);
  RC(sle_proprio_fwd_multi(sv, nullptr, ni, kKeep, n, c->HW, 512, nc, (long)n * c->HW * 512, c->cam.stride, nD, nD, 0, st));
  // bottleneck Dense (K-split) -> LayerNorm -> tanh per camera, side by side in enc[i]
  const int S0 = split_under(n, kBottleneck, nc * ni, 32);
  GemmDesc g0[2];
  LnFwdArgs l0[2];
  for (int i = 0; i < ni; ++i) {
    g0[i] = layer_fwd(c->cam.dense, P, train_cam_io(c, n, i), n, t->slabs + (long)i * nc * S0 * n * kBottleneck, S0);
    l0[i] = layer_ln_fwd(c->cam.dense, P, train_cam_io(c, n, i), n, g0[i]);
  }
  RC(gemm_f32_multi(g0, ni, st));
  RC(ln_fwd_multi(l0, ni, kBottleneck, st));
  // classifier head: Dense_0 (K-split) of both instances, then the row kernel
  const int S1 = split_under(n, kHidden, ni, 8);
  GemmDesc g1[2];
  for (int i = 0; i < ni; ++i)
    g1[i] = gemm_fwd(t->enc + (long)i * n * c->E, c->E, 0, P + c->o_w1, 0, t->slabs + (long)i * S1 * n * kHidden, 1, n, kHidden, c->E, S1);
  RC(gemm_f32_multi(g1, ni, st));
  ClsHeadArgs h{};
  h.slabs = t->slabs; h.S = S1; h.sstride = (long)n * kHidden; h.istride = (long)S1 * n * kHidden;
  h.b1 = P + c->o_b1; h.g1 = P + c->o_g1; h.be1 = P + c->o_be1; h.w2 = P + c->o_w2; h.b2 = P + c->o_b2;
  h.n = n; h.keep = kKeep;
  h.mask = masks ? masks + (long)nc * nD : nullptr;
  if (!masks) { h.gen = 1; h.key[0] = keys[2 * nc]; h.key[1] = keys[2 * nc + 1]; }
  h.labels = labels; h.logits = t->logits;
  h.xhat = t->hxhat; h.dg = t->hdg; h.dz = t->dz; h.dw2in = t->dw2in; h.dlogit = t->dlogit; h.rowloss = t->rowloss; h.rowcorr = t->rowcorr;
  hipLaunchKernelGGL(cls_head_kernel, dim3(cdiv(n, 4), ni), dim3(256), 0, st, h);
  SERL_HIP(hipGetLastError());
  return SERL_OK;
}

int check_train(serl_classifier* c, int n) {
  SERL_REQUIRE(c, "NULL classifier");
  if (!c->tr) {
    serl::set_error("classifier training is not initialised (serl_classifier_train_init)");
    return SERL_ERR_STATE;
  }
  SERL_REQUIRE(n >= 1 && n <= c->tr->max_batch, "n = %d not in [1, training max_batch = %d]", n, c->tr->max_batch);
  return SERL_OK;
}

int resolve_moment(serl_classifier* c, const char* section, const char* leaf, float** ptr, long* count) {
  SERL_REQUIRE(section && leaf, "NULL argument");
  const Leaf* l = find(c->leaves, leaf);
  SERL_REQUIRE(l, "unknown classifier leaf '%s'", leaf);
  *count = l->count;
  SERL_REQUIRE(c->tr->opt.moment(section, *l, ptr), "unknown classifier section '%s' (opt/mu, opt/nu)", section);
  return SERL_OK;
}

}  // namespace

extern "C" {

int serl_classifier_train_init(serl_classifier* c, int max_batch, float lr, float b1, float b2, float eps) {
  SERL_REQUIRE(c, "NULL classifier");
  SERL_REQUIRE(!c->tr, "classifier training is already initialised");
  SERL_REQUIRE(max_batch >= 1 && lr > 0.f, "bad training max_batch %d / learning rate %g", max_batch, (double)lr);
  SERL_REQUIRE(b1 == 0.9f && b2 == 0.999f && eps == 1e-8f, "only optax.adam's defaults b1 = 0.9, b2 = 0.999, eps = 1e-8 are implemented");
  SERL_HIP(hipSetDevice(c->cfg.device));
  ClsTrain* t = new ClsTrain();
  t->max_batch = max_batch;
  t->lr = lr;
  if (int rc = alloc_zeroed(&t->arena, carve_train(c, t, nullptr), "classifier training arena")) {
    delete t;
    return rc;
  }
  carve_train(c, t, (uint8_t*)t->arena);
  c->tr = t;
  return SERL_OK;
}

int serl_classifier_train_forward(serl_classifier* c, const uint8_t* dev_frames, int n, const uint8_t* dev_masks,
                                  const uint32_t* host_mask_keys, float* dev_logits, void* stream) {
  RC(check_train(c, n));
  SERL_REQUIRE(dev_frames && dev_logits && (dev_masks || host_mask_keys), "NULL argument (the Dropout needs keep-masks or keys)");
  hipStream_t st = (hipStream_t)stream;
  SERL_HIP(hipSetDevice(c->cfg.device));
  RC(train_forward(c, dev_frames, n, nullptr, dev_masks, host_mask_keys, false, st));
  SERL_HIP(hipMemcpyAsync(dev_logits, c->tr->logits, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
  return SERL_OK;
}

int serl_classifier_train_step(serl_classifier* c, const uint8_t* dev_frames, int n, const float* dev_labels,
                               const uint8_t* dev_masks, const uint32_t* host_mask_keys, void* stream) {
  RC(check_train(c, n));
  SERL_REQUIRE(dev_frames && dev_labels && (dev_masks || host_mask_keys), "NULL argument (the Dropout needs keep-masks or keys)");
  const serl_classifier_cfg& g = c->cfg;
  ClsTrain* t = c->tr;
  hipStream_t st = (hipStream_t)stream;
  SERL_HIP(hipSetDevice(g.device));
  const float* P = c->params;
  float* G = t->opt.grad();   // G[o] = gradient of the leaf at arena offset o
  const int nc = g.n_cam;
  const long nD = (long)n * c->D;
  RC(train_forward(c, dev_frames, n, dev_labels, dev_masks, host_mask_keys, true, st));
  hipLaunchKernelGGL(cls_info_kernel, dim3(1), dim3(256), 0, st, t->rowloss, t->rowcorr, n, t->info);
  SERL_HIP(hipGetLastError());
  // d enc = dz W1^T
  const GemmDesc gi = gemm_igrad(t->dz, kHidden, 0, P + c->o_w1, kHidden, 0, t->denc, c->E, 0, 1, n, c->E, kHidden);
  RC(gemm_f32_multi(&gi, 1, st));
  // camera heads: tanh + LayerNorm backward (all cameras), then d f = dzc W^T per camera
  const DenseLn& cam = c->cam.dense;
  const DenseLnIo tc = train_cam_io(c, n, 0);
  const DenseLnGrad dc{t->denc, c->E, kBottleneck, t->dzc, t->dgc};
  RC(ln_bwd(layer_ln_bwd(cam, P, tc, dc, n), st));
  const GemmDesc gf = layer_igrad(cam, P, dc, n, t->df, c->D, nD);
  RC(gemm_f32_multi(&gf, 1, st));
  // through the camera Dropout, then the SpatialLearnedEmbeddings kernels' gradient (batch splits summed by the last arriver)
  ClsDropArgs da{};
  da.df = t->df; da.per_cam = nD; da.mask = dev_masks; da.keep = kKeep;
  if (!dev_masks)
    for (int k = 0; k < nc; ++k) { da.key[k][0] = host_mask_keys[2 * k]; da.key[k][1] = host_mask_keys[2 * k + 1]; }
  hipLaunchKernelGGL(cls_dropout_bwd_kernel, dim3(cdiv(nD, 256), nc), dim3(256), 0, st, da);
  SERL_HIP(hipGetLastError());
  const long sle_n = (long)c->HW * 512 * kSleFeatures;
  RC(sle_bwd_fused(t->feats, t->df, t->sle_part, n, c->HW, 512, kSleSplit, nc, (long)n * c->HW * 512, nD, kSleSplit * sle_n,
                   G + c->cam.first, c->cam.stride, t->ctr, st));
  // every other parameter gradient: one column-sum launch and one grouped weight-gradient GEMM
  const Colsum3Args cs[4] = {
      {t->hdg, t->hxhat, t->dz, 1, n, kHidden, G + c->o_g1, G + c->o_be1, G + c->o_b1, 0, 0},
      {t->dw2in, nullptr, nullptr, 1, n, kHidden, nullptr, G + c->o_w2, nullptr, 0, 1},
      {t->dlogit, nullptr, nullptr, 1, n, 1, nullptr, G + c->o_b2, nullptr, 0, 2},
      layer_colsum(cam, tc, dc, n, G),
  };
  RC(colsum3_multi(cs, 4, st));
  const GemmDesc wg[2] = {
      gemm_wgrad(t->enc, c->E, 0, t->dz, kHidden, 0, G + c->o_w1, kHidden, 0, 1, c->E, kHidden, n),   // dDense_0 = enc^T dz
      layer_wgrad(cam, tc, dc, n, G),                                                                  // per camera dDense = f^T dzc
  };
  RC(gemm_f32_multi(wg, 2, st));
  // optax.adam(lr) (reward_classifier.py:62-66) over the trainable slice
  return t->opt.apply(c->params, t->lr, st);
}

int serl_classifier_read_train_info(serl_classifier* c, float out[2], void* stream) {
  RC(check_train(c, 1));
  SERL_REQUIRE(out, "NULL argument");
  SERL_HIP(hipSetDevice(c->cfg.device));
  SERL_HIP(hipMemcpyAsync(out, c->tr->info, 2 * sizeof(float), hipMemcpyDefault, (hipStream_t)stream));
  return SERL_OK;
}

int serl_classifier_train_set_step(serl_classifier* c, int64_t step) {
  RC(check_train(c, 1));
  SERL_REQUIRE(step >= 0, "negative step");
  c->tr->opt.step = step;
  return SERL_OK;
}

int serl_classifier_train_get_step(serl_classifier* c, int64_t* step_out) {
  RC(check_train(c, 1));
  SERL_REQUIRE(step_out, "NULL argument");
  *step_out = c->tr->opt.step;
  return SERL_OK;
}

int serl_classifier_train_set(serl_classifier* c, const char* section, const char* leaf, const float* host, int64_t count) {
  RC(check_train(c, 1));
  SERL_REQUIRE(host, "NULL argument");
  float* p = nullptr;
  long n = 0;
  RC(resolve_moment(c, section, leaf, &p, &n));
  SERL_REQUIRE(count == n, "leaf '%s' has %ld elements, got %ld", leaf, n, (long)count);
  SERL_HIP(hipSetDevice(c->cfg.device));
  return leaf_copy(p, host, n, hipMemcpyHostToDevice, section, leaf, kFrozenMoment);
}

int serl_classifier_train_get(serl_classifier* c, const char* section, const char* leaf, float* host_out, int64_t count) {
  RC(check_train(c, 1));
  SERL_REQUIRE(host_out, "NULL argument");
  float* p = nullptr;
  long n = 0;
  RC(resolve_moment(c, section, leaf, &p, &n));
  SERL_REQUIRE(count == n, "leaf '%s' has %ld elements, got %ld", leaf, n, (long)count);
  SERL_HIP(hipSetDevice(c->cfg.device));
  return leaf_copy(host_out, p, n, hipMemcpyDeviceToHost, section, leaf, kFrozenMoment);
}

}  // extern "C"
