// Behaviour cloning (serl_launcher/agents/continuous/bc.py, built by utils/launcher.py:26-47 with
// encoder_type="resnet-pretrained"): parameter arena, update, inference and the serl_bc half of the C ABI.
//   Policy(EncodingWrapper(use_proprio=True, enable_stacking=True), MLP([256, 256], tanh, no LayerNorm, activate_final),
//          tanh_squash_distribution=False, std = clip(exp(log_std), 1e-5, 5) * sqrt(temperature))
//   (networks/actor_critic_nets.py:167-227, networks/mlp.py, common/encoding.py:26-72)
// Policy calls its encoder with stop_gradient=True, and EncodingWrapper stops the gradient of every image branch
// (encoding.py:48-49): only the proprio Dense/LayerNorm, the two MLP layers and the two heads train.  The frozen trunk, the
// SpatialLearnedEmbeddings and the bottleneck Dense/LayerNorm of every camera run forward only; their Adam moments are zero
// forever (Adam with g = m = v = 0 leaves a parameter unchanged) and are produced on read instead of stored.
// Reuses the trunk (trunk_f16x3.hip) and the encoder-head / GEMM / Adam kernels (heads.hip); new here: the bias + tanh slab
// reduction of a plain Dense -> tanh layer, its backward, and the diagonal-Gaussian NLL head.
// serl_bc_opts.no_proprio: EncodingWrapper(use_proprio=False), BCAgent.create's own default -- the code is the image codes alone,
// no proprio leaves or launches, and only the two MLP layers and the two heads train.
#include <cmath>
#include <string>
#include <vector>

#include "dense_layer.h"
#include "jaxrng.h"

using namespace serl;

namespace {
constexpr int kHidden = 256, kBottleneck = 256, kSleFeatures = 8, kProprio = 64, kMaxAct = 64;
}  // namespace

struct serl_bc {
  serl_bc_cfg cfg{};
  bool has_prop = true;   // the proprio branch (serl_bc_opts.no_proprio == 0); else the state is never read
  int HW = 0, D = 0, Eimg = 0, E = 0;
  std::vector<Leaf> leaves;    // trunk, cameras (frozen), then the trainable slice [t0, t0 + nt)
  long n_params = 0, t0 = 0, nt = 0;
  TrunkOffsets to{};
  CamHeadOffsets cam{};
  DenseLn prop{};   // the proprio branch
  long o_w1 = 0, o_b1 = 0, o_w2 = 0, o_b2 = 0, o_Wm = 0, o_bm = 0, o_Ws = 0, o_bs = 0;
  void* arena = nullptr;
  float* params = nullptr;   // [n_params + 1]: the element behind the trainable slice is adam_ema's (unused) temperature slot
  AdamSlice opt{};           // moments, gradient and update count of the trainable slice
  TrunkWeights tw{};
  TrunkWorkspace tws{};
  TrunkPacked tpk{};
  float *feats = nullptr, *f = nullptr, *slabs = nullptr, *enc = nullptr, *pxhat = nullptr, *prstd = nullptr;
  float *h1 = nullptr, *h2 = nullptr, *mu = nullptr, *dhead = nullptr, *dpre1 = nullptr, *dpre2 = nullptr;
  float *dprop = nullptr, *dpp = nullptr, *dgp = nullptr, *info = nullptr;
  long slabs_cap = 0;
};

namespace {

void layout(serl_bc* c) {
  const serl_bc_cfg& g = c->cfg;
  const TrunkDims d = trunk_dims(g.H, g.W);
  c->HW = d.h[5] * d.w[5];
  c->D = 512 * kSleFeatures;
  c->Eimg = kBottleneck * g.n_cam;
  c->E = c->Eimg + (c->has_prop ? kProprio : 0);
  std::vector<Leaf>& L = c->leaves;
  long off = 0;
  c->to = add_trunk_leaves(L, off);
  c->cam = add_cam_head_leaves(L, off, g.n_cam, c->D, kBottleneck, [&](const std::string& p) { add_leaf(L, off, p + "sle", (long)c->HW * 512 * kSleFeatures); });
  off = (off + 3) & ~3L;   // (16-byte aligned trainable slice)
  c->t0 = off;
  const long A = g.act_dim;
  if (c->has_prop) c->prop = add_dense_ln_leaves(L, off, "enc/proprio/dense/kernel", "enc/proprio/dense/bias", "enc/proprio/ln", 1, g.state_dim, kProprio, kActTanh);
  c->o_w1 = add_leaf(L, off, "actor/w1", (long)c->E * kHidden);
  c->o_b1 = add_leaf(L, off, "actor/b1", kHidden);
  c->o_w2 = add_leaf(L, off, "actor/w2", (long)kHidden * kHidden);
  c->o_b2 = add_leaf(L, off, "actor/b2", kHidden);
  c->o_Wm = add_leaf(L, off, "actor/mean/kernel", kHidden * A);
  c->o_bm = add_leaf(L, off, "actor/mean/bias", A);
  c->o_Ws = add_leaf(L, off, "actor/logstd/kernel", kHidden * A);
  c->o_bs = add_leaf(L, off, "actor/logstd/bias", A);
  c->nt = off - c->t0;
  c->n_params = off;
}

size_t carve(serl_bc* c, uint8_t* base) {
  const serl_bc_cfg& g = c->cfg;
  Bump b(base);
  const long n = g.max_batch, A = g.act_dim, np = c->has_prop ? n : 0;   // np: rows of proprio scratch
  c->params = b.take<float>(c->n_params + 1);
  c->opt.carve(b, c->t0, c->nt);
  c->info = b.take<float>(2);
  uint8_t* pk = b.take<uint8_t>(trunk_packed_bytes());
  uint8_t* ws = b.take<uint8_t>(trunk_workspace_bytes(g.n_cam * g.max_batch, g.H, g.W));
  c->feats = b.take<float>((size_t)g.n_cam * n * c->HW * 512);
  c->f = b.take<float>((size_t)g.n_cam * n * c->D);
  c->slabs_cap = (long)std::max(32 * g.n_cam, 8) * n * kBottleneck;
  c->slabs = b.take<float>(c->slabs_cap);
  c->enc = b.take<float>(n * c->E);
  c->pxhat = b.take<float>(np * kProprio);
  c->prstd = b.take<float>(np);
  c->h1 = b.take<float>(n * kHidden);
  c->h2 = b.take<float>(n * kHidden);
  c->mu = b.take<float>(n * A);
  c->dhead = b.take<float>(2 * n * A);
  c->dpre1 = b.take<float>(n * kHidden);
  c->dpre2 = b.take<float>(n * kHidden);
  c->dprop = b.take<float>(np * kProprio);
  c->dpp = b.take<float>(np * kProprio);
  c->dgp = b.take<float>(np * kProprio);
  if (base) {
    trunk_packed_bind(c->tpk, pk);
    trunk_workspace_bind(c->tws, ws, g.n_cam * g.max_batch, g.H, g.W);
    c->tw = trunk_weights(c->params, c->to);
  }
  return b.off;
}

// ---- new kernels ------------------------------------------------------------------------------
// Plain Dense -> tanh (mlp.py:26-34 with use_layer_norm=False): y[r][c] = tanh(bias[c] + sum_s slab[s][r][c]), the K-split
// GEMM's slabs reduced in index order.  Takes the place of the LayerNorm launch of the DrQ MLP layer.
__global__ __launch_bounds__(256) void bc_dense_tanh_fwd_kernel(const float* slabs, int S, long sstride, const float* bias,
                                                                 float* y, int rows, int N) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)rows * N) return;
  const int col = (int)(e % N);
  float acc = 0.f;
  for (int s = 0; s < S; ++s) acc += slabs[(long)s * sstride + e];
  y[e] = tanhf(acc + bias[col]);
}

// Its backward: the input gradient of the layer above arrives as `S` slabs (K-split / per-head products);
// dpre = (sum_s slab[s]) * (1 - y^2).  The bias gradient is colsum3 mode 1 of dpre (deferred to the end of the step).
__global__ __launch_bounds__(256) void bc_dense_tanh_bwd_kernel(const float* slabs, int S, long sstride, const float* y,
                                                                 float* dpre, int rows, int N) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)rows * N) return;
  float acc = 0.f;
  for (int s = 0; s < S; ++s) acc += slabs[(long)s * sstride + e];
  const float t = y[e];
  dpre[e] = acc * (1.f - t * t);
}

// Diagonal-Gaussian head (distrax.MultivariateNormalDiag, actor_critic_nets.py:188-221 with tanh_squash_distribution=False):
// mean = bias_m + sum of the mean slabs, log_std = bias_s + sum of the log-std slabs, std = clip(exp(log_std), lo, hi) * sqrt(T).
// One workgroup; rows are strided over the threads and every batch sum is a fixed-order tree (deterministic).
struct BcHeadArgs {
  const float* slabs; int S; long sstride;   // [2 (mean, log_std)][S][B][A]
  const float *bias_m, *bias_s;
  int B, A; float std_min, std_max, temp;
  const float* action;                        // [B][A] or nullptr
  float* mu;                                  // [B][A] mode (or nullptr)
  float *logp, *mse;                          // per-sample [B] (or nullptr)
  float *dmu, *dls;                           // d(-mean log_prob) / d(mean, log_std) [B][A] (or nullptr)
  float* info;                                // [2]: -mean(log_prob), mean(mse) (or nullptr)
  float* act; const float* eps;               // act = mu (+ std * eps when `sample`)
  int sample, tf; uint32_t tf_key[2];         // tf: eps[b][j] = jax.random.normal(tf_key, (B, A))[b][j]
};
__global__ __launch_bounds__(256) void bc_gauss_head_kernel(BcHeadArgs a) {
  __shared__ float red[2][256];
  const int tid = threadIdx.x;
  const float half_log_2pi = 0.918938533204672742f;   // 0.5 * log(2 pi)
  const float sq = sqrtf(a.temp);
  float s_lp = 0.f, s_mse = 0.f;
  for (int b = tid; b < a.B; b += 256) {
    float lp = 0.f, se = 0.f;
    for (int j = 0; j < a.A; ++j) {
      const long e = (long)b * a.A + j;
      float pm = 0.f, ps = 0.f;
      for (int s = 0; s < a.S; ++s) {
        pm += a.slabs[(long)s * a.sstride + e];
        ps += a.slabs[(long)(a.S + s) * a.sstride + e];
      }
      const float mean = pm + a.bias_m[j], ls = ps + a.bias_s[j];
      const float raw = expf(ls);
      const float sd = fminf(fmaxf(raw, a.std_min), a.std_max) * sq;
      if (a.mu) a.mu[e] = mean;
      if (a.act) {
        float out = mean;
        if (a.sample) {
          const float z = a.tf ? normal_from_bits(random_bits_at(a.tf_key[0], a.tf_key[1], (uint64_t)a.B * a.A, (uint64_t)e)) : a.eps[e];
          out = mean + sd * z;
        }
        a.act[e] = out;
      }
      if (a.action) {
        const float d = a.action[e] - mean;
        const float z = d / sd;
        lp += -0.5f * z * z - logf(sd) - half_log_2pi;
        se += d * d;
        // actor_loss = -mean_b sum_j log N(a | mean, sd): no gradient where the clip is active (as policy_dist_bwd)
        if (a.dmu) a.dmu[e] = -(z / sd) / (float)a.B;
        if (a.dls) a.dls[e] = (raw > a.std_min && raw < a.std_max) ? -(z * z - 1.f) / (float)a.B : 0.f;
      }
    }
    if (a.action) {
      if (a.logp) a.logp[b] = lp;
      if (a.mse) a.mse[b] = se;
      s_lp += lp;
      s_mse += se;
    }
  }
  if (!a.info) return;
  red[0][tid] = s_lp;
  red[1][tid] = s_mse;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) { red[0][tid] += red[0][tid + o]; red[1][tid] += red[1][tid + o]; }
    __syncthreads();
  }
  if (tid == 0) {
    a.info[0] = -red[0][0] / (float)a.B;
    a.info[1] = red[1][0] / (float)a.B;
  }
}

int dense_tanh_fwd(const float* slabs, int S, long sstride, const float* bias, float* y, int rows, int N, hipStream_t st) {
  hipLaunchKernelGGL(bc_dense_tanh_fwd_kernel, dim3(cdiv((long)rows * N, 256)), dim3(256), 0, st, slabs, S, sstride, bias, y, rows, N);
  SERL_HIP(hipGetLastError());
  return SERL_OK;
}

int dense_tanh_bwd(const float* slabs, int S, long sstride, const float* y, float* dpre, int rows, int N, hipStream_t st) {
  hipLaunchKernelGGL(bc_dense_tanh_bwd_kernel, dim3(cdiv((long)rows * N, 256)), dim3(256), 0, st, slabs, S, sstride, y, dpre, rows, N);
  SERL_HIP(hipGetLastError());
  return SERL_OK;
}

// ---- forward ---------------------------------------------------------------------------------
// Policy forward (actor_critic_nets.py:179-190) on n observations up to the head GEMM's slabs: one frozen-trunk pass over the
// n_cam * n images, SpatialLearnedEmbeddings (+ Dropout keep-mask: injected, drawn from per-camera jax.random keys, or none at
// train=False) with the proprio branch riding on the same launch, bottleneck Dense + LayerNorm + tanh, the two Dense -> tanh
// layers and the two heads.  Returns the head's K-split count.
// the proprio branch's tensors: reads `state`, writes the columns of the code behind the cameras'
DenseLnIo prop_io(const serl_bc* c, const float* state) {
  return DenseLnIo{state, c->cfg.state_dim, 0, c->enc + c->Eimg, c->E, 0, c->pxhat, c->prstd};
}

int forward(serl_bc* c, const uint8_t* frames, const float* state, int n, const uint8_t* mask, const uint32_t* mask_keys,
            int* head_split, hipStream_t st) {
  const serl_bc_cfg& g = c->cfg;
  const float* P = c->params;
  const int A = g.act_dim;
  RC(trunk_forward(c->tw, c->tws, frames, g.n_cam * n, c->feats, st, &c->tpk));
  SleFwdArgs sv{};
  sv.x = c->feats; sv.K = P + c->cam.first; sv.mask = mask; sv.f = c->f;
  if (!mask && mask_keys) sle_tf_masks(sv, mask_keys, g.n_cam, n, 0);
  ProprioArgs pv{};
  if (c->has_prop) pv = layer_row_fwd(c->prop, P, prop_io(c, state));
  RC(sle_proprio_fwd_multi(&sv, c->has_prop ? &pv : nullptr, 1, 1.0f - g.dropout, n, c->HW, 512, g.n_cam, (long)n * c->HW * 512, c->cam.stride,
                           (long)n * c->D, (long)n * c->D, g.state_dim, st));
  // bottleneck Dense (K-split) -> LayerNorm -> tanh per camera, side by side in enc
  const int S0 = split_under(n, kBottleneck, g.n_cam, 32);
  const DenseLnIo tc{c->f, c->D, (long)n * c->D, c->enc, c->E, kBottleneck, nullptr, nullptr};
  const GemmDesc g0 = layer_fwd(c->cam.dense, P, tc, n, c->slabs, S0);
  const LnFwdArgs l0 = layer_ln_fwd(c->cam.dense, P, tc, n, g0);
  RC(gemm_f32_multi(&g0, 1, st));
  RC(ln_fwd_multi(&l0, 1, kBottleneck, st));
  // MLP: Dense(256) -> tanh, twice (activate_final) -- no LayerNorm, so not the DenseLn layer: GEMM forms written out
  const int S1 = split_under(n, kHidden, 1, 8);
  const GemmDesc g1 = gemm_fwd(c->enc, c->E, 0, P + c->o_w1, 0, c->slabs, 1, n, kHidden, c->E, S1);
  RC(gemm_f32_multi(&g1, 1, st));
  RC(dense_tanh_fwd(c->slabs, S1, g1.sCz, P + c->o_b1, c->h1, n, kHidden, st));
  const int S2 = split_under(n, kHidden, 1, 4);
  const GemmDesc g2 = gemm_fwd(c->h1, kHidden, 0, P + c->o_w2, 0, c->slabs, 1, n, kHidden, kHidden, S2);
  RC(gemm_f32_multi(&g2, 1, st));
  RC(dense_tanh_fwd(c->slabs, S2, g2.sCz, P + c->o_b2, c->h2, n, kHidden, st));
  // heads: Dense_0 (mean) and Dense_1 (log_std) as the two batches of one GEMM
  const int S3 = 4;
  const GemmDesc g3 = gemm_fwd(c->h2, kHidden, 0, P + c->o_Wm, c->o_Ws - c->o_Wm, c->slabs, 2, n, A, kHidden, S3);
  RC(gemm_f32_multi(&g3, 1, st));
  *head_split = S3;
  return SERL_OK;
}

BcHeadArgs head_args(serl_bc* c, int n, int S) {
  BcHeadArgs h{};
  h.slabs = c->slabs; h.S = S; h.sstride = (long)n * c->cfg.act_dim;
  h.bias_m = c->params + c->o_bm; h.bias_s = c->params + c->o_bs;
  h.B = n; h.A = c->cfg.act_dim; h.std_min = c->cfg.std_min; h.std_max = c->cfg.std_max; h.temp = 1.0f;
  return h;
}

int launch_head(const BcHeadArgs& h, hipStream_t st) {
  hipLaunchKernelGGL(bc_gauss_head_kernel, dim3(1), dim3(256), 0, st, h);
  SERL_HIP(hipGetLastError());
  return SERL_OK;
}

int check_batch(serl_bc* c, const serl_batch* b) {
  const serl_bc_cfg& g = c->cfg;
  SERL_REQUIRE(b && b->frames && (b->state || !c->has_prop) && b->action, "serl_batch has NULL members");
  SERL_REQUIRE(b->batch >= 1 && b->batch <= g.max_batch, "batch %d not in [1,%d]", b->batch, g.max_batch);
  SERL_REQUIRE(b->n_cam == g.n_cam && b->H == g.H && b->W == g.W && b->C == 3 && b->state_dim == g.state_dim &&
                   b->act_dim == g.act_dim, "serl_batch shape does not match the BC agent");
  SERL_REQUIRE(b->num_stack <= 1, "the BC agent takes single-frame observations (serl_batch.num_stack %d)", b->num_stack);
  return SERL_OK;
}

// (section, leaf) -> device pointer; nullptr: a frozen leaf's Adam moment (always zero, not stored)
int resolve(serl_bc* c, const char* section, const char* leaf, float** ptr, long* count) {
  const Leaf* l = find(c->leaves, leaf);
  SERL_REQUIRE(l, "unknown BC leaf '%s'", leaf);
  *count = l->count;
  if (std::string(section) == "params") { *ptr = c->params + l->off; return SERL_OK; }
  SERL_REQUIRE(c->opt.moment(section, *l, ptr), "unknown BC section '%s' (params, opt/mu, opt/nu)", section);
  return SERL_OK;
}

}  // namespace

extern "C" {

int serl_bc_create(const serl_bc_cfg* cfg, serl_bc** out) {
  const serl_bc_opts opts{};
  return serl_bc_create_opts(cfg, &opts, out);
}

int serl_bc_use_proprio(serl_bc* c) { return c ? (c->has_prop ? 1 : 0) : -1; }

int serl_bc_create_opts(const serl_bc_cfg* cfg, const serl_bc_opts* opts, serl_bc** out) {
  SERL_REQUIRE(cfg && opts && out, "NULL argument");
  SERL_REQUIRE(opts->no_proprio == 0 || opts->no_proprio == 1, "no_proprio %d is not 0 (the proprio branch) or 1 (image codes alone)", opts->no_proprio);
  SERL_REQUIRE(cfg->n_cam >= 1 && cfg->n_cam <= SERL_MAX_CAMS, "n_cam %d not in [1,%d]", cfg->n_cam, SERL_MAX_CAMS);
  SERL_REQUIRE(cfg->H >= 32 && cfg->W >= 32 && cfg->max_batch >= 1, "bad BC shape");
  SERL_REQUIRE(cfg->state_dim >= 1 && cfg->act_dim >= 1 && cfg->act_dim <= kMaxAct, "state_dim %d / act_dim %d unsupported",
               cfg->state_dim, cfg->act_dim);
  SERL_REQUIRE(cfg->dropout >= 0.f && cfg->dropout < 1.f && cfg->std_min > 0.f && cfg->std_max > cfg->std_min, "bad BC hyper-parameters");
  SERL_HIP(hipSetDevice(cfg->device));
  serl_bc* c = new serl_bc();
  c->cfg = *cfg;
  c->has_prop = !opts->no_proprio;
  layout(c);
  if (int rc = alloc_zeroed(&c->arena, carve(c, nullptr), "BC arena")) {
    delete c;
    return rc;
  }
  carve(c, (uint8_t*)c->arena);
  *out = c;
  return SERL_OK;
}

int serl_bc_destroy(serl_bc* c) {
  if (!c) return SERL_OK;
  if (c->arena) (void)hipFree(c->arena);
  delete c;
  return SERL_OK;
}

int serl_bc_num_leaves(serl_bc* c) { return c ? (int)c->leaves.size() : 0; }

int serl_bc_leaf_info(serl_bc* c, int i, char* name_out, int name_cap, int64_t* count, int* trainable) {
  SERL_REQUIRE(c && i >= 0 && i < (int)c->leaves.size(), "leaf index %d out of range", i);
  const Leaf& l = c->leaves[i];
  if (name_out && name_cap > 0) snprintf(name_out, name_cap, "%s", l.name.c_str());
  if (count) *count = l.count;
  if (trainable) *trainable = l.off >= c->t0 ? 1 : 0;
  return SERL_OK;
}

int serl_bc_set(serl_bc* c, const char* section, const char* leaf, const float* host, int64_t count) {
  SERL_REQUIRE(c && section && leaf && host, "NULL argument");
  float* p = nullptr;
  long n = 0;
  RC(resolve(c, section, leaf, &p, &n));
  SERL_REQUIRE(count == n, "leaf '%s' has %ld elements, got %ld", leaf, n, (long)count);
  SERL_HIP(hipSetDevice(c->cfg.device));
  RC(leaf_copy(p, host, n, hipMemcpyHostToDevice, section, leaf, kFrozenMoment));
  if (std::string(leaf).rfind("trunk/", 0) == 0 && std::string(section) == "params") c->tpk.dirty = true;
  return SERL_OK;
}

int serl_bc_get(serl_bc* c, const char* section, const char* leaf, float* host_out, int64_t count) {
  SERL_REQUIRE(c && section && leaf && host_out, "NULL argument");
  float* p = nullptr;
  long n = 0;
  RC(resolve(c, section, leaf, &p, &n));
  SERL_REQUIRE(count == n, "leaf '%s' has %ld elements, got %ld", leaf, n, (long)count);
  SERL_HIP(hipSetDevice(c->cfg.device));
  return leaf_copy(host_out, p, n, hipMemcpyDeviceToHost, section, leaf, kFrozenMoment);
}

int serl_bc_set_step(serl_bc* c, int64_t step) {
  SERL_REQUIRE(c && step >= 0, "bad step");
  c->opt.step = step;
  return SERL_OK;
}

int64_t serl_bc_get_step(serl_bc* c) { return c ? c->opt.step : -1; }

int serl_bc_update(serl_bc* c, const serl_batch* batch, const uint8_t* dev_masks, const uint32_t* host_mask_keys, void* stream) {
  SERL_REQUIRE(c, "NULL BC agent");
  RC(check_batch(c, batch));
  SERL_REQUIRE(dev_masks || host_mask_keys, "the Dropout of the update needs keep-masks or jax.random keys");
  const serl_bc_cfg& g = c->cfg;
  SERL_HIP(hipSetDevice(g.device));
  hipStream_t st = (hipStream_t)stream;
  const int n = batch->batch, A = g.act_dim;
  const float* P = c->params;
  float* G = c->opt.grad();   // G[o] = gradient of the trainable leaf at arena offset o
  int S3 = 0;
  RC(forward(c, batch->frames, batch->state, n, dev_masks, host_mask_keys, &S3, st));
  // loss, info and the head gradients (bc.py:44-68)
  BcHeadArgs h = head_args(c, n, S3);
  h.action = batch->action; h.mu = c->mu;
  h.dmu = c->dhead; h.dls = c->dhead + (long)n * A; h.info = c->info;
  RC(launch_head(h, st));
  // dh2 = dmu Wm^T + dls Ws^T: the two products as slabs, summed by the tanh backward of layer 2
  const GemmDesc gh = gemm_igrad(c->dhead, A, (long)n * A, P + c->o_Wm, A, c->o_Ws - c->o_Wm, c->slabs, kHidden, (long)n * kHidden, 2, n, kHidden, A);
  RC(gemm_f32_multi(&gh, 1, st));
  RC(dense_tanh_bwd(c->slabs, 2, gh.sCz, c->h2, c->dpre2, n, kHidden, st));
  // dh1 = dpre2 W2^T (K-split slabs) -> dpre1
  const int S2 = split_under(n, kHidden, 1, 4);
  const GemmDesc gd = gemm_igrad(c->dpre2, kHidden, 0, P + c->o_w2, kHidden, 0, c->slabs, kHidden, (long)n * kHidden, 1, n, kHidden, kHidden, S2);
  RC(gemm_f32_multi(&gd, 1, st));
  RC(dense_tanh_bwd(c->slabs, S2, gd.sCz, c->h1, c->dpre1, n, kHidden, st));
  // gradient of the proprio code only (the image codes are behind stop_gradient): dpre1 W1[Eimg:E]^T
  // (without the proprio branch the policy has no trainable input: no such GEMM, LayerNorm backward or gradient entry)
  const int np = c->has_prop ? 5 : 4;   // entries of the two gradient launches
  const DenseLnIo tp = c->has_prop ? prop_io(c, batch->state) : DenseLnIo{};
  const DenseLnGrad dp{c->dprop, kProprio, 0, c->dpp, c->dgp};
  if (c->has_prop) {
    const GemmDesc gp = gemm_igrad(c->dpre1, kHidden, 0, P + c->o_w1 + (long)c->Eimg * kHidden, kHidden, 0, c->dprop, kProprio, 0, 1, n, kProprio, kHidden);
    RC(gemm_f32_multi(&gp, 1, st));
    RC(ln_bwd(layer_ln_bwd(c->prop, P, tp, dp, n), st));
  }
  // every parameter gradient: one column-sum launch and one grouped weight-gradient GEMM
  const float* dmu = c->dhead;
  const float* dls = c->dhead + (long)n * A;
  const Colsum3Args cs[5] = {
      {c->dpre1, nullptr, nullptr, 1, n, kHidden, nullptr, G + c->o_b1, nullptr, 0, 1},
      {c->dpre2, nullptr, nullptr, 1, n, kHidden, nullptr, G + c->o_b2, nullptr, 0, 1},
      {dmu, nullptr, nullptr, 1, n, A, nullptr, G + c->o_bm, nullptr, 0, 1},
      {dls, nullptr, nullptr, 1, n, A, nullptr, G + c->o_bs, nullptr, 0, 1},
      c->has_prop ? layer_colsum(c->prop, tp, dp, n, G) : Colsum3Args{},
  };
  RC(colsum3_multi(cs, np, st));
  auto wg = [&](const float* X, long ldx, const float* dY, long ldy, float* out, int Mx, int Ny) {
    return gemm_wgrad(X, ldx, 0, dY, ldy, 0, out, Ny, 0, 1, Mx, Ny, n);
  };
  const GemmDesc wgs[5] = {
      wg(c->enc, c->E, c->dpre1, kHidden, G + c->o_w1, c->E, kHidden),
      wg(c->h1, kHidden, c->dpre2, kHidden, G + c->o_w2, kHidden, kHidden),
      wg(c->h2, kHidden, dmu, A, G + c->o_Wm, kHidden, A),
      wg(c->h2, kHidden, dls, A, G + c->o_Ws, kHidden, A),
      c->has_prop ? layer_wgrad(c->prop, tp, dp, n, G) : GemmDesc{},
  };
  RC(gemm_f32_multi(wgs, np, st));
  // optax.adam(lr) over the trainable slice (bc.py:139 via common.py:170-220); one count, no schedule, no clip
  return c->opt.apply(c->params, g.lr, st);
}

int serl_bc_read_info(serl_bc* c, float out[2], void* stream) {
  SERL_REQUIRE(c && out, "NULL argument");
  SERL_HIP(hipSetDevice(c->cfg.device));
  SERL_HIP(hipMemcpyAsync(out, c->info, 2 * sizeof(float), hipMemcpyDefault, (hipStream_t)stream));
  return SERL_OK;
}

int serl_bc_sample_actions(serl_bc* c, const uint8_t* dev_frames, const float* dev_state, int n, const float* dev_eps,
                           const uint32_t* host_key, float temperature, int argmax, float* dev_actions_out, void* stream) {
  SERL_REQUIRE(c && dev_frames && (dev_state || !c->has_prop) && dev_actions_out, "NULL argument");
  SERL_REQUIRE(n >= 1 && n <= c->cfg.max_batch, "n = %d not in [1, max_batch = %d]", n, c->cfg.max_batch);
  SERL_REQUIRE(argmax || dev_eps || host_key, "sampling needs eps or a jax.random key");
  SERL_REQUIRE(temperature >= 0.f, "negative temperature");
  SERL_HIP(hipSetDevice(c->cfg.device));
  hipStream_t st = (hipStream_t)stream;
  int S3 = 0;
  RC(forward(c, dev_frames, dev_state, n, nullptr, nullptr, &S3, st));
  BcHeadArgs h = head_args(c, n, S3);
  h.temp = temperature;
  h.act = dev_actions_out;
  h.sample = argmax ? 0 : 1;
  h.eps = dev_eps;
  if (!argmax && !dev_eps) { h.tf = 1; h.tf_key[0] = host_key[0]; h.tf_key[1] = host_key[1]; }
  return launch_head(h, st);
}

int serl_bc_debug_metrics(serl_bc* c, const serl_batch* batch, float* dev_mse, float* dev_logp, float* dev_pi, void* stream) {
  SERL_REQUIRE(c && dev_mse && dev_logp && dev_pi, "NULL argument");
  RC(check_batch(c, batch));
  SERL_HIP(hipSetDevice(c->cfg.device));
  hipStream_t st = (hipStream_t)stream;
  const int n = batch->batch;
  int S3 = 0;
  RC(forward(c, batch->frames, batch->state, n, nullptr, nullptr, &S3, st));
  BcHeadArgs h = head_args(c, n, S3);
  h.action = batch->action; h.mu = dev_pi; h.logp = dev_logp; h.mse = dev_mse;
  return launch_head(h, st);
}

}  // extern "C"
