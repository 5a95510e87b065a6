// Host-callable launchers of heads.hip (internal, not part of the C ABI).
#pragma once
#include <cmath>

#include "internal.h"

namespace serl {

extern long g_chain_launches;   // kernels launched by heads.hip since the library was loaded (diagnostic)

// The update chain is a long sequence of small dependent kernels, each costing ~5 us of launch/drain latency
// whatever its size: independent instances of the same kind of work (the three EncodingWrapper passes of a
// loss, the online and target critics, the two policy evaluations of the actor step) share one launch.
constexpr int kMaxMulti = 4;
template <typename T>
struct Multi { T v[kMaxMulti]; };
constexpr int kMaxGemmGroups = 6;
int gemm_f32_multi(const GemmDesc* groups, int n, hipStream_t stream);  // same operand layout in every group

int reduce_slabs(const float* slabs, int S, long slab_stride, int groups, int rows, int N, const float* bias,
                 long bias_gstride, float* out, long ld_out, long out_gstride, bool accumulate,
                 hipStream_t stream, float scale = 1.0f);

// D: the row width of every instance, a multiple of 64 in [64, 1024] (one wave per row, D / 64 columns per lane)
// RAGGED rows (an instance's d != 0; all instances of a launch or none): the row's true width is d < D and columns [d, D) are zero
// padding -- of the bias, scale, shift and of the kernel's columns, hence of the slabs.  The statistics divide by d; everything else
// is the on-grid row, which leaves y == 0 in the pads (gamma == beta == 0 and act(0) == 0).  The backward divides by d and writes
// dx = 0 in the pads (the on-grid row would leave rstd * (-m1 - xhat * m2) there).  Plain rows need neither.  No Dropout.
// Instances without gamma and beta are LayerNorm-free MLP layers (mlp.py:29-30; plain_row): y = act(bias + slabs), the same riders,
// the pre-activation in xhat, rstd not written.  All instances of a launch are plain or none is; plain ones carry no Dropout.
int ln_fwd_multi(const LnFwdArgs* a, int n, int D, hipStream_t stream);
// One width-256 ReLU instance with a row-dot (the reward classifier's head), closed for reward labelling: dot_out = logits,
// label[row] = sigmoid(logit) >= 0.5, mean[0] = the labels' mean, summed in a fixed order inside the launch (ctr: one zeroed
// arrival counter)
int label_rows(const LnFwdArgs& a, float* label, float* mean, int* ctr, hipStream_t stream);

// REDQ target + critic loss as a rider workgroup of the LayerNorm-backward launch that consumes dQ (sac.py:142-191)
struct RedqSel { int n; int idx[16]; };
struct LossArgs {
  int on;
  const float *qt, *q, *reward, *mask; RedqSel sel; int E, B; float discount, inv_norm;
  float *y_out, *dq, *scalars, *dbias; int per_member; const float *logp_next, *alpha;
};
struct LnBwdArgs {
  const float* dy; long ld_dy; long dy_goff;  // same addressing as LnFwdArgs::y (ignored in rank-1 mode)
  // rank-1 mode (gradient through the critic head): dy[row][col] = (dq ? dq[row] : dq_const) * dq_w[col]
  const float* dq; const float* dq_w; float dq_const;
  long dq_w_gstride;  // 0: shared head vector; else per-group head vectors
  const float* y; long ld_y; long y_goff;
  const float* xhat; const float* rstd;
  const float* gamma; long pstride;
  int rows, rows_per_group;
  float* dx;  // [rows][D] gradient wrt the pre-activation
  float* dg;  // [rows][D] dy * act'(pre): dy*(1-y^2) for tanh  (-> dbeta = colsum(dg), dgamma = colsum(dg*xhat))
  int act;            // kAct* of the forward row (per instance, uniform over a wave)
  int d;              // as LnFwdArgs::d: 0, or the true width of a zero-padded row (in the hole behind act)
  const float* beta;  // kActSwish only: the forward's beta (addressed like gamma), to recompute pre = gamma*xhat + beta
  int D;          // the row width, a multiple of 64 in [64, 1024]
  int dq_inline;  // rank-1 mode: dq[row] = 2 (q - y) inv_norm computed from the LossArgs of the launch
  LnDrop drop;    // the forward row's Dropout, stated again: dx = keep-decision ? dx / keep : 0 (zero-initialised: none)
};
// up to kMaxMulti LayerNorm backward passes in one launch (+ the critic-loss rider when loss.on).  Widths 64 and 256 may share a
// launch (the encoder heads); any other width (an MLP layer at hidden != 256) must be the width of every instance.  One
// instance of width 64 or 256 without a rider takes a launch of its own kind with one LnBwdArgs for arguments.
// Instances without gamma are LayerNorm-free MLP layers (mlp.py:29-30, use_layer_norm=False; plain_bwd_row): dx = dy * act'(.) from y
// and, for swish, the pre-activation the forward row kept in xhat; rstd, beta and dg are not touched (dg == dx).  All instances
// of a launch are plain or none is; plain ones share one width and carry no Dropout.
int ln_bwd_multi(const LnBwdArgs* a, int n, const LossArgs& loss, hipStream_t stream);
inline int ln_bwd(const LnBwdArgs& a, hipStream_t stream) { return ln_bwd_multi(&a, 1, LossArgs{}, stream); }

int colsum(const float* X, const float* Y, int groups, int rows_per_group, int D, float* out,
           long out_gstride, bool accumulate, hipStream_t stream);
struct Colsum3Args {
  const float *dg, *xhat, *dpre; int groups, rows_per_group, D;
  float *o_gamma, *o_beta, *o_bias; long gstride;
  int mode;   // 0: the three sums of a Dense->LN->tanh layer; 1: o_beta[g][j] = sum_r dg[r][j] only (bias gradient of a plain
              // Dense); 2: o_beta[0] = sum_r dg[r] (a vector's sum: rows_per_group elements, D = groups = 1)
};
constexpr int kMaxColsum = 8;
int colsum3_multi(const Colsum3Args* layers, int n, hipStream_t stream);
int colsum3(const float* dg, const float* xhat, const float* dpre, int groups, int rows_per_group, int D,
            float* o_gamma, float* o_beta, float* o_bias, long gstride, hipStream_t stream);
struct SleFwdArgs {
  const float* x; const float* K; const uint8_t* mask; float* f;
  // sle_proprio_fwd only: mask == nullptr && gen -> Dropout keep-mask hashed from (seed, camera, GLOBAL row, channel)
  // gen == 2: jax.random.bernoulli(tf_key[camera], keep, (tf_rows, channels * 8))[tf_row0 + row][...] instead of the hash (jaxrng.h)
  int gen; uint64_t seed; long row_offset, rows_global;
  uint32_t tf_key[4][2]; long tf_rows, tf_row0;
};
// SpatialLearnedEmbeddings channel-blocked (a workgroup = 256 channels x 8 samples: the kernel K is read once per workgroup,
// not once per sample) + inline Dropout mask + the proprio branch as extra workgroups of the same launch (pv == nullptr: none).
// pv whose instances have no `state` (an agent without the proprio branch): the extra workgroups carry the instances' column-copy
// riders alone -- all instances of a launch have a state or none has; the caller passes nullptr where no instance has a rider
struct ProprioArgs;
int sle_proprio_fwd_multi(const SleFwdArgs* v, const ProprioArgs* pv, int n, float keep, int N, int HW, int Cc, int groups, long x_gs,
                          long k_gs, long mask_gs, long f_gs, int state_dim, hipStream_t stream);
int sle_fwd_multi(const SleFwdArgs* v, int n, float keep_scale, int N, int HW, int Cc, int groups, long x_gs, long k_gs,
                  long mask_gs, long f_gs, hipStream_t stream);
int sle_bwd(const float* x, const float* df, float* partial, int N, int HW, int Cc, int nsplit, int groups,
            long x_gs, long df_gs, long part_gs, hipStream_t stream);
// the same with the sum over the batch splits done by the last-arriving workgroup of every (camera, pixel, channel block):
// out[g][hw][c][j] (camera stride out_gs) -- no reduce_slabs launch.  ctr: groups * HW * cdiv(Cc, 256) zeroed counters.
int sle_bwd_fused(const float* x, const float* df, float* partial, int N, int HW, int Cc, int nsplit, int groups,
                  long x_gs, long df_gs, long part_gs, float* out, long out_gs, int* ctr, hipStream_t stream);
// dbias: gradient of the head bias -- one scalar (shared head) or, with per_member_bias, one per ensemble member.
// sel: the target ensemble members whose minimum backs up (sac.py:150-161: critic_subsample_size random members, n = 0: all).
// logp_next / alpha != nullptr: backup_entropy (sac.py:174-176): y -= alpha[0] * logp_next[b]
int critic_loss(const float* qt, const float* q, const float* reward, const float* mask, RedqSel sel, int E,
                int B, float discount, float inv_norm, float* y_out, float* dq, float* scalars, float* dbias,
                hipStream_t stream, bool per_member_bias = false, const float* logp_next = nullptr, const float* alpha = nullptr);
int policy_dist_fwd_multi(const PolicyDistArgs* v, int n, int B, int A, float std_min, float std_max, hipStream_t stream);
// The policy distribution of `rows` rows read off the head GEMM's slabs (the layout policy_dist_fwd_multi reads), without a
// sample: loc, scale_diag, mode and -- with `act` [rows][A] -- log pi(act | s) (sac.py:71-91).  Any output may be nullptr; logp
// needs act.  A row with an action component |a| >= 1 under the tanh squash gets a non-finite logp (not clamped).
struct PolicyStatsArgs {
  const float* slabs; int S;   // [mean | log_std][S K-splits][rows][A]; kPolUniform: [mean] alone, bias_ls = log_stds;
                               // kPolFixed: [mean] alone, bias_ls = fixed_std
  const float *bias_mean, *bias_ls, *act;
  float *mean, *std, *mode_out, *logp;   // [rows][A] x 3, [rows]
  int rows, A; float std_min, std_max;
  int mode;   // kPol*
};
int policy_stats(const PolicyStatsArgs& v, hipStream_t stream);
// proprio branch: y = tanh(LN(state W + b)) with W [S][64] (encoding.py:55-70), one wave per row
struct ProprioArgs {
  const float* state; const float *W, *b, *gamma, *beta;
  float* y; long ld_y; float* xhat; float* rstd;
  const float* copy_src; long ld_copy_src; float* copy_dst; long ld_copy_dst; int copy_cols;  // optional rider
};
int proprio_fwd_multi(const ProprioArgs* v, int n, int S, int rows, hipStream_t stream);
int policy_dist_bwd(const float* da, long ld_da, const float* act, long ld_act, const float* pre,
                    const float* stdv, const float* eps, const float* alpha, float coef, int B, int A,
                    float std_min, float std_max, float* dpre, const float* q, int E, float* qmean_out,
                    hipStream_t stream, int mode = kPolExp);  // rider: qmean_out[0] = sum_b mean_e q[e][b]; mode: kPol*
struct CopyJob { const float* src; long ld_src; float* dst; long ld_dst; int cols; };
int copy_cols_multi(const CopyJob* jobs, int n, int rows, hipStream_t stream);
int fill(float* p, float v, long n, hipStream_t stream);

struct AdamArgs {
  float *theta, *theta_target;
  long P, Pc, Pa0, Pa1;  // critic-tx support [0,Pc), actor-tx support [Pa0,Pa1), temperature = P-1
  const float *g_critic, *g_actor;
  float *m_c, *v_c, *m_a, *v_a, *m_t, *v_t;
  const float* sum_logp_next;  // device scalar: local/all-reduced sum of log pi(next)
  float* temp_grad_out;        // device scalar (debug/export)
  int critic_on, actor_on, temp_on;
  float lr_c, lr_a, lr_t, bc1, bc2, tau, target_entropy, inv_batch;
  // target EMA (common.py:124-134) runs when ema_on; optimizers with *_on == 0 step with a zero gradient
  int ema_on;
  // optional make_optimizer branches (optimizers.py:32-46); all zero = plain adam
  float wd_c, wd_a, wd_t;           // adamw weight decay of each optimizer (applies to EVERY leaf of the tree)
  float clip_c, clip_a, clip_t;     // clip_by_global_norm thresholds (<= 0: none)
  const float* norm2;               // device [2]: squared global norm of g_critic / g_actor (when a clip is active)
  // frozen (trunk) leaves appended to the index space: target EMA, and weight decay if any optimizer has one
  float* frozen; float* frozen_target; long n_frozen;
  long n_frozen_live; int vec_ok;   // set by adam_ema(): frozen leaves this launch covers; the 4-wide fast path may be used
  // info rider: 0 = none, 1 = critic step, 2 = actor/temperature step.  Slot order of `scalars` / `info_acc` as in
  // agent.hip (S_* / I_* enums); info_acc has 8 floats.
  int info_mode, info_reset;
  const float* scalars; const float* alpha; float* info_acc;
  float info_w, inv_eb;
};
int adam_ema(const AdamArgs& a, hipStream_t stream);
// the info rider of `a` alone (info_mode, scalars, alpha, info_acc, ...): no parameter, moment or target is read or written
int adam_info_only(const AdamArgs& a, hipStream_t stream);
// optax.adam(lr) alone over a trainable slice theta[0, nt) (no schedule, clip or target), at update number `step` (1-based).
// m / v hold nt + 1 floats: the last is the temperature slot adam_ema keeps at P - 1, never touched (g = m = v = 0).
inline AdamArgs adam_slice(float* theta, long nt, const float* g, float* m, float* v, float lr, int64_t step) {
  AdamArgs a{};
  a.theta = theta; a.theta_target = nullptr;
  a.P = nt + 1; a.Pc = 0; a.Pa0 = 0; a.Pa1 = nt;
  a.g_actor = g; a.m_a = m; a.v_a = v;
  a.m_t = m + nt; a.v_t = v + nt;
  a.actor_on = 1;
  a.lr_a = lr;
  a.bc1 = 1.0f - powf(0.9f, (float)step);
  a.bc2 = 1.0f - powf(0.999f, (float)step);
  return a;
}
// optax.adam(lr) over the trainable slice [t0, t0 + nt) of a parameter vector whose leaves in front of t0 are frozen (BC, the
// reward classifier): the moments and the gradient of the slice alone, and the update count.  A frozen leaf's moments are zero
// forever (Adam with g = m = v = 0 leaves a parameter unchanged): not stored, produced on read (leaf_copy).
constexpr const char* kFrozenMoment = "'%s' of the frozen leaf '%s' must be zero";
struct AdamSlice {
  long t0 = 0, nt = 0;
  float *m = nullptr, *v = nullptr, *G = nullptr;   // [nt + 1], [nt + 1], [nt]
  int64_t step = 0;
  void carve(Bump& b, long t0_, long nt_) {
    t0 = t0_; nt = nt_;
    m = b.take<float>(nt + 1);
    v = b.take<float>(nt + 1);
    G = b.take<float>(nt);
  }
  float* grad() const { return G - t0; }   // grad()[o] = gradient of the trainable leaf at arena offset o
  // section "opt/mu" / "opt/nu" (anything else: false) -> *ptr = that moment of leaf `l`, nullptr for a frozen leaf
  bool moment(const char* section, const Leaf& l, float** ptr) const {
    const std::string s = section;
    if (s != "opt/mu" && s != "opt/nu") return false;
    *ptr = l.off < t0 ? nullptr : (s == "opt/mu" ? m : v) + (l.off - t0);
    return true;
  }
  int apply(float* params, float lr, hipStream_t stream) {   // one update of params[t0, t0 + nt) from G
    RC(adam_ema(adam_slice(params + t0, nt, G, m, v, lr, step + 1), stream));
    step += 1;
    return SERL_OK;
  }
};
// `steps` target-EMA steps of frozen leaves in one pass (exactly the values `steps` adam_ema launches would have left)
int frozen_ema(const float* frozen, float* frozen_target, long n, float tau, long steps, hipStream_t stream);
// out[0] = sum g_critic^2 over [0, nc), out[1] = sum g_actor^2 over [0, na) (deterministic single-block reduction)
int grad_norm2(const float* g_critic, long nc, const float* g_actor, long na, float* out, hipStream_t stream);
// kind 0: N(0,1) f32, 1: keep-mask u8.  The tensor is [planes][rows_local][row_elems]; the value of an element is a
// hash of its position in the GLOBAL tensor [planes][rows_global][row_elems] (rows row_offset.. of it), so that a
// batch-sharded job draws the same noise for a sample whichever rank owns it (rows_global == 0: local == global)
struct NoiseJob { void* out; long n; uint64_t seed; int kind; float keep; long rows_local, rows_global, row_offset, row_elems; };
int gen_noise_multi(const NoiseJob* v, int n, hipStream_t stream);

// ---- the three GEMM forms of a Dense layer, for `groups` independent (input, kernel) pairs `*_gs` floats apart ------------------
// Forward Y = X W as `splitk` K-split slabs: X [rows][K] (row stride ldx), W [K][N] row-major; the slab of (group g, split s) is
// the [rows][N] block g * splitk + s behind `slabs`.
inline GemmDesc gemm_fwd(const float* X, long ldx, long x_gs, const float* W, long w_gs, float* slabs, int groups, int rows, int N,
                         int K, int splitk) {
  GemmDesc g{};
  g.A = X; g.sAm = ldx; g.sAk = 1; g.sAb = x_gs;
  g.B = W; g.sBk = N; g.sBn = 1; g.sBb = w_gs;
  g.C = slabs; g.ldc = N; g.sCz = (long)rows * N;
  g.M = rows; g.N = N; g.K = K; g.nbatch = groups; g.splitk = splitk;
  return g;
}
// Input gradient dX = dY W^T: dY [rows][Nout] (row stride ldy), W [Kin][Nout] (row stride ldw); block z (= group * splitk + split)
// of the result lands at out + z * out_zs with row stride ldo.
inline GemmDesc gemm_igrad(const float* dY, long ldy, long dy_gs, const float* W, long ldw, long w_gs, float* out, long ldo,
                           long out_zs, int groups, int rows, int Kin, int Nout, int splitk = 1) {
  GemmDesc g{};
  g.A = dY; g.sAm = ldy; g.sAk = 1; g.sAb = dy_gs;
  g.B = W; g.sBk = 1; g.sBn = ldw; g.sBb = w_gs;
  g.C = out; g.ldc = ldo; g.sCz = out_zs;
  g.M = rows; g.N = Kin; g.K = Nout; g.nbatch = groups; g.splitk = splitk;
  return g;
}
// Weight gradient dW = X^T dY, written in place: X [rows][Mx] (row stride ldx), dY [rows][Ny] (row stride ldy), group g's
// [Mx][Ny] result (row stride ldo) at out + g * out_gs.
inline GemmDesc gemm_wgrad(const float* X, long ldx, long x_gs, const float* dY, long ldy, long dy_gs, float* out, long ldo,
                           long out_gs, int groups, int Mx, int Ny, int rows) {
  GemmDesc g{};
  g.A = X; g.sAm = 1; g.sAk = ldx; g.sAb = x_gs;
  g.B = dY; g.sBk = ldy; g.sBn = 1; g.sBb = dy_gs;
  g.C = out; g.ldc = ldo; g.sCz = out_gs;
  g.M = Mx; g.N = Ny; g.K = rows; g.nbatch = groups; g.splitk = 1;
  return g;
}

// Dropout keep-masks of the SpatialLearnedEmbeddings launch drawn from host jax.random keys [n_cam][2]: rows row0.. of
// jax.random.bernoulli(key, keep, (rows, D)) per camera.
inline void sle_tf_masks(SleFwdArgs& s, const uint32_t* keys, int n_cam, long rows, long row0) {
  s.gen = 2;
  for (int k = 0; k < n_cam; ++k) { s.tf_key[k][0] = keys[2 * k]; s.tf_key[k][1] = keys[2 * k + 1]; }
  s.tf_rows = rows; s.tf_row0 = row0;
}

}  // namespace serl
