// The WIDE head rows: every kernel that touches an action vector, for action widths 64 < A <= 256 (serl_agent_opts.wide_actions).
// The narrow kernels of heads.hip give one lane of a wave to one action column and stay what they are for A <= 64; their host
// launchers hand a launch with A > 64 over to the kernels below, one for one.  Device code and its launchers; included once by
// heads.hip, inside namespace serl, behind the narrow kernels whose helpers it shares (policy_std, policy_ls_group, softplusf,
// hash_normal, ln_gather, fanout_row).
//
// Row layout -- that of the width-generic LayerNorm rows (ln_row, STRIDED).  One wave owns one sample row; lane l holds the
// columns l + 64 j for j < nb = ceil(A / 64) <= 4, so every load and store instruction of a wave covers 64 consecutive floats
// (256 bytes) whatever A is.  A block j >= nb does not exist for the wave: a branch on a launch argument, uniform over the wave.
// In the last block a lane past A is predicated by DESIGN.md section 8's rule: its address is clamped to the row's last column
// (head_col), the load is unconditional, the value it forms is selected to exactly 0 before any sum and its stores are skipped.
// No lane reads or writes outside its row.  All loads of a row are issued before its first store.
//
// Row sums (log pi, the Tanh bijector's log-determinant): a lane adds the terms of its columns over j in index order, then the
// xor butterfly of the wave (head_wave_sum).  The order depends on A alone -- not on the grid, not on the row count, not on where
// the row stands -- so a row's bits are the same in a launch of 1 row and in one of 65.
//
// No LDS (the critic fan-out keeps the 16 KB of the narrow kernel it widens), no scratch; at most 4 columns per lane.
#pragma once

constexpr int kHeadWideMax = 256;   // the widest action row: 4 blocks of 64 columns
constexpr int kHeadNb = kHeadWideMax / 64;

// a lane's column in block j and whether the row has it; the address of a column past A is the row's last
__device__ __forceinline__ int head_col(int lane, int j, int A, bool& live) {
  const int col = lane + 64 * j;
  live = col < A;
  return live ? col : A - 1;
}
__device__ __forceinline__ float head_wave_sum(float s) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) s += __shfl_xor(s, off);
  return s;
}
// the terms of log pi at one column: the Gaussian's from the draw z (= (u - mean) / std), the squash's from u
template <int MODE>
__device__ __forceinline__ float head_logp_term(float z, float log_sd, float u) {
  float t = -0.5f * z * z - log_sd - 0.91893853320467274f;
  if (!(MODE & kPolNoTanh)) t -= 2.f * (0.69314718055994531f - u - softplusf(-2.f * u));
  return t;
}
// mean and `ls` (log-std, softplus argument, or with kPolFixed the std itself) of a lane's columns from the head GEMM's K-split
// slabs, per column by the arithmetic of policy_dist_rows: the bias first, then the slabs in index order.  off = the row's first
// element in slab 0 of the mean's group; the log-std group lies S slabs behind.
template <int MODE>
__device__ __forceinline__ void head_gather(const float* slabs, int S, long slab_stride, long off, const float* bias_mean,
                                            const float* bias_ls, int nb, const int (&cc)[kHeadNb], float (&mean)[kHeadNb],
                                            float (&ls)[kHeadNb]) {
#pragma unroll
  for (int j = 0; j < kHeadNb; ++j) {
    mean[j] = ls[j] = 0.f;
    if (j < nb) { mean[j] = bias_mean[cc[j]]; ls[j] = bias_ls[cc[j]]; }
  }
  for (int sp = 0; sp < S; ++sp) {
    const long o0 = off + (long)sp * slab_stride, o1 = o0 + (long)S * slab_stride;
#pragma unroll
    for (int j = 0; j < kHeadNb; ++j) {
      if (j < nb) {
        mean[j] += slabs[o0 + cc[j]];
        if (policy_ls_group<MODE>()) ls[j] += slabs[o1 + cc[j]];
      }
    }
  }
}

// =============================================================================================
// Policy head forward (the work of policy_dist_fwd_kernel and of the kEpiPolicy epilogue): blockIdx.y = instance, a wave per row.
// Sums the slabs, takes the std, reads eps or draws it -- element row * A + col of the threefry / hashed stream, as the narrow
// kernels index it -- and writes the action at its leading dimension, pre, std_out, eps_out (drawn noise alone), logp[row] and
// alpha_out.  sum_logp is not written: the caller sums logp in the vector-sum job of colsum3 (the order of the narrow kernels).
// =============================================================================================
template <int MODE>
__global__ __launch_bounds__(256) void policy_head_wide_kernel(Multi<PolicyDistArgs> mv) {
  const PolicyDistArgs& v = mv.v[blockIdx.y];
  if (blockIdx.x == 0 && threadIdx.x == 0 && v.alpha_out) v.alpha_out[0] = softplusf(v.lam[0]);
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= v.B) return;   // (uniform over the wave)
  const int A = v.A, nb = (A + 63) >> 6;
  int cc[kHeadNb];
  bool live[kHeadNb];
#pragma unroll
  for (int j = 0; j < kHeadNb; ++j) cc[j] = head_col(lane, j, A, live[j]);
  float mean[kHeadNb], ls[kHeadNb], ep[kHeadNb];
  head_gather<MODE>(v.slabs, v.S, v.slab_stride, (long)row * v.slab_ld, v.bias_mean, v.bias_ls, nb, cc, mean, ls);
  const long rb = (long)row * A;
#pragma unroll
  for (int j = 0; j < kHeadNb; ++j) {
    ep[j] = 0.f;
    if (j < nb) {
      if (v.eps) ep[j] = v.eps[rb + cc[j]];
      else
        ep[j] = v.tf ? normal_from_bits(random_bits_at(v.tf_key[0], v.tf_key[1], (uint64_t)v.tf_rows * (uint64_t)A,
                                                       (uint64_t)(v.tf_row0 + row) * (uint64_t)A + (uint64_t)cc[j]))
                     : hash_normal(v.seed, (uint64_t)(v.row_offset + row) * (uint64_t)A + (uint64_t)cc[j]);
    }
  }
  float lp = 0.f;
#pragma unroll
  for (int j = 0; j < kHeadNb; ++j) {
    if (j < nb) {
      const float sd = policy_std<MODE>(ls[j], v.std_min, v.std_max);
      const float u = mean[j] + sd * ep[j];
      if (live[j]) {
        const long e = rb + cc[j];
        if (!v.eps) v.eps_out[e] = ep[j];
        v.pre[e] = mean[j];
        if (!policy_fixed<MODE>()) v.pre[(long)v.B * A + e] = ls[j];
        v.act[(long)row * v.ld_act + cc[j]] = (MODE & kPolNoTanh) ? u : tanhf(u);
        v.std_out[e] = sd;
      }
      const float t = head_logp_term<MODE>(ep[j], logf(sd), u);
      lp += live[j] ? t : 0.f;
    }
  }
  lp = head_wave_sum(lp);
  if (lane == 0) v.logp[row] = lp;
}

int policy_head_wide_fwd(const Multi<PolicyDistArgs>& mv, int n, int B, hipStream_t stream) {
  const dim3 grid(cdiv(B, 4), n);
#define SERL_X(M) SERL_LAUNCH_CHAIN(policy_head_wide_kernel<M>, grid, dim3(256), 0, stream, mv)
  SERL_POLICY_MODE_SWITCH(mv.v[0].mode, SERL_X, SERL_REQUIRE(false, "bad policy distribution mode %d", mv.v[0].mode))
#undef SERL_X
  SERL_HIP(hipGetLastError());
  return SERL_OK;
}

// =============================================================================================
// Policy head backward (the work of policy_dist_bwd_kernel, its expressions per element): the (1 - a^2) factor, the clip gates,
// dpre [2][B][A] ([1][B][A] with kPolFixed).  The column sums of dpre -- the bias gradients and, with kPolUniform, the gradient of
// log_stds -- are colsum's, which takes any width.  The last workgroup is the rider of the narrow kernel: sum_b mean_e Q[e][b].
// =============================================================================================
struct HeadBwdArgs {
  const float* da; long ld_da; const float* act; long ld_act;
  const float *pre, *stdv, *eps, *alpha; float coef; int B, A; float std_min, std_max;
  float* dpre; const float* q; int E; float* qmean_out;
};
template <int MODE>
__global__ __launch_bounds__(256) void policy_head_wide_bwd_kernel(HeadBwdArgs v) {
  const int B = v.B, A = v.A;
  if (blockIdx.x == gridDim.x - 1) {   // rider (one extra workgroup), in the narrow kernel's order
    __shared__ float red[256];
    float sacc = 0.f;
    for (int b = threadIdx.x; b < B; b += 256) {
      float m = 0.f;
      for (int e = 0; e < v.E; ++e) m += v.q[(long)e * B + b];
      sacc += m / (float)v.E;
    }
    red[threadIdx.x] = sacc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
      __syncthreads();
    }
    if (threadIdx.x == 0) v.qmean_out[0] = red[0];
    return;
  }
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= B) return;   // (uniform over the wave)
  const int nb = (A + 63) >> 6;
  const long rb = (long)row * A;
  const float c_lp = v.alpha[0] * v.coef;
  int cc[kHeadNb];
  bool live[kHeadNb];
  float gu[kHeadNb], a[kHeadNb], sd[kHeadNb], ls[kHeadNb], ep[kHeadNb];
#pragma unroll
  for (int j = 0; j < kHeadNb; ++j) {
    cc[j] = head_col(lane, j, A, live[j]);
    gu[j] = a[j] = ls[j] = ep[j] = 0.f;
    sd[j] = 1.f;
    if (j < nb) {
      gu[j] = v.da[(long)row * v.ld_da + cc[j]];
      if (!(MODE & kPolNoTanh)) a[j] = v.act[(long)row * v.ld_act + cc[j]];
      if (!policy_fixed<MODE>()) {
        sd[j] = v.stdv[rb + cc[j]];
        ls[j] = v.pre[(long)B * A + rb + cc[j]];
        ep[j] = v.eps[rb + cc[j]];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < kHeadNb; ++j) {
    if (j < nb && live[j]) {
      const long e = rb + cc[j];
      float g = gu[j];
      if (!(MODE & kPolNoTanh)) g = g * (1.f - a[j] * a[j]) + c_lp * 2.f * a[j];
      v.dpre[e] = g;
      if (!policy_fixed<MODE>()) {
        const float raw = policy_std_raw<MODE>(ls[j]);
        const float dstd = g * ep[j] - c_lp / sd[j];
        const float draw = (MODE & kPolStdMask) == kPolSoftplus ? 1.f / (1.f + expf(-ls[j])) : sd[j];   // d raw / d ls
        v.dpre[(long)B * A + e] = (raw > v.std_min && raw < v.std_max) ? dstd * draw : 0.f;
      }
    }
  }
}

int policy_head_wide_bwd(const HeadBwdArgs& v, int mode, hipStream_t stream) {
#define SERL_X(M) SERL_LAUNCH_CHAIN(policy_head_wide_bwd_kernel<M>, dim3(cdiv(v.B, 4) + 1), dim3(256), 0, stream, v)
  SERL_POLICY_MODE_SWITCH(mode, SERL_X, SERL_REQUIRE(false, "bad policy distribution mode %d", mode))
#undef SERL_X
  SERL_HIP(hipGetLastError());
  return SERL_OK;
}

// =============================================================================================
// Inspection rows (the work of policy_stats_kernel and policy_stats_fixed_kernel): loc / scale / mode and log pi(act | s) with
// the atanh pre-image, not clamped: a component with |a| >= 1 makes the row's log-density non-finite, as the reference's is.
// =============================================================================================
template <int MODE>
__global__ __launch_bounds__(256) void policy_stats_wide_kernel(PolicyStatsArgs v) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= v.rows) return;   // (uniform over the wave)
  const int A = v.A, nb = (A + 63) >> 6;
  const long rb = (long)row * A;
  int cc[kHeadNb];
  bool live[kHeadNb];
#pragma unroll
  for (int j = 0; j < kHeadNb; ++j) cc[j] = head_col(lane, j, A, live[j]);
  float mean[kHeadNb], ls[kHeadNb], a[kHeadNb];
  head_gather<MODE>(v.slabs, v.S, (long)v.rows * A, rb, v.bias_mean, v.bias_ls, nb, cc, mean, ls);
#pragma unroll
  for (int j = 0; j < kHeadNb; ++j) a[j] = (v.act && j < nb) ? v.act[rb + cc[j]] : 0.f;
  float lp = 0.f;
#pragma unroll
  for (int j = 0; j < kHeadNb; ++j) {
    if (j < nb) {
      const float sd = policy_std<MODE>(ls[j], v.std_min, v.std_max);
      if (v.logp) {   // (uniform: a launch argument)
        float u = a[j];
        if (!(MODE & kPolNoTanh)) u = 0.5f * (log1pf(a[j]) - log1pf(-a[j]));
        const float t = head_logp_term<MODE>((u - mean[j]) / sd, logf(sd), u);
        lp += live[j] ? t : 0.f;
      }
      if (live[j]) {
        if (v.mean) v.mean[rb + cc[j]] = mean[j];
        if (v.std) v.std[rb + cc[j]] = sd;
        if (v.mode_out) v.mode_out[rb + cc[j]] = (MODE & kPolNoTanh) ? mean[j] : tanhf(mean[j]);
      }
    }
  }
  if (v.logp) {
    lp = head_wave_sum(lp);
    if (lane == 0) v.logp[row] = lp;
  }
}

int policy_stats_wide(const PolicyStatsArgs& v, hipStream_t stream) {
#define SERL_X(M) SERL_LAUNCH_CHAIN(policy_stats_wide_kernel<M>, dim3(cdiv(v.rows, 4)), dim3(256), 0, stream, v)
  SERL_POLICY_MODE_SWITCH(v.mode, SERL_X, SERL_REQUIRE(false, "bad policy distribution mode %d", v.mode))
#undef SERL_X
  SERL_HIP(hipGetLastError());
  return SERL_OK;
}

// =============================================================================================
// N samples per row (the work of policy_fanout_kernel): the wave sums the slabs once and keeps mean, std and log std of its
// columns -- 12 registers -- while it loops over the row's candidates, kHeadCj at a time: the eps loads of a pass (kHeadCj * nb,
// each 256 consecutive bytes at candidate stride rows * A) are issued together, the butterflies of its log-densities interleave.
// A pass past the last candidate repeats the last one's addresses and stores nothing.
// =============================================================================================
constexpr int kHeadCj = 4;
template <int MODE>
__global__ __launch_bounds__(256) void policy_fanout_wide_kernel(PolicyFanoutArgs v) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= v.rows) return;   // (uniform over the wave)
  const int A = v.A, N = v.N, nb = (A + 63) >> 6;
  const long rb = (long)row * A, cstride = (long)v.rows * A;
  int cc[kHeadNb];
  bool live[kHeadNb];
#pragma unroll
  for (int j = 0; j < kHeadNb; ++j) cc[j] = head_col(lane, j, A, live[j]);
  float mean[kHeadNb], sd[kHeadNb], lsd[kHeadNb];
  head_gather<MODE>(v.slabs, v.S, cstride, rb, v.bias_mean, v.bias_ls, nb, cc, mean, sd);
#pragma unroll
  for (int j = 0; j < kHeadNb; ++j) {
    sd[j] = policy_std<MODE>(sd[j], v.std_min, v.std_max);
    lsd[j] = logf(sd[j]);
  }
  for (int c0 = 0; c0 < N; c0 += kHeadCj) {
    float z[kHeadCj][kHeadNb], lp[kHeadCj];
#pragma unroll
    for (int c = 0; c < kHeadCj; ++c) {
      const float* ep = v.eps + (long)min(c0 + c, N - 1) * cstride + rb;
#pragma unroll
      for (int j = 0; j < kHeadNb; ++j) z[c][j] = j < nb ? ep[cc[j]] : 0.f;
    }
#pragma unroll
    for (int c = 0; c < kHeadCj; ++c) {
      float* out = v.actions + ((long)row * N + min(c0 + c, N - 1)) * A;
      lp[c] = 0.f;
#pragma unroll
      for (int j = 0; j < kHeadNb; ++j) {
        if (j < nb) {
          const float u = mean[j] + sd[j] * z[c][j];
          if (live[j] && c0 + c < N) out[cc[j]] = (MODE & kPolNoTanh) ? u : tanhf(u);
          const float t = head_logp_term<MODE>(z[c][j], lsd[j], u);
          lp[c] += live[j] ? t : 0.f;
        }
      }
    }
    if (v.logp) {   // (uniform: a launch argument)
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
        for (int c = 0; c < kHeadCj; ++c) lp[c] += __shfl_xor(lp[c], off);
      }
      float mine = 0.f;
#pragma unroll
      for (int c = 0; c < kHeadCj; ++c) mine = lane == c ? lp[c] : mine;
      if (lane < kHeadCj && c0 + lane < N) v.logp[(long)row * N + c0 + lane] = mine;
    }
  }
}

int policy_fanout_wide(const PolicyFanoutArgs& v, hipStream_t stream) {
#define SERL_X(M) SERL_LAUNCH_CHAIN(policy_fanout_wide_kernel<M>, dim3(cdiv(v.rows, 4)), dim3(256), 0, stream, v)
  SERL_POLICY_MODE_SWITCH(v.mode, SERL_X, SERL_REQUIRE(false, "bad policy distribution mode %d", v.mode))
#undef SERL_X
  SERL_HIP(hipGetLastError());
  return SERL_OK;
}

// =============================================================================================
// The best of N candidates (q_rank_kernel's ranking, expression for expression: members in ascending order, ties to the lowest
// j, a candidate's index whatever the scores are) with the winner's copy over the row layout: up to 4 columns per lane.
// =============================================================================================
__global__ __launch_bounds__(256) void q_rank_wide_kernel(QRankArgs v) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= v.n) return;   // (uniform over the wave)
  const int N = v.N, E = v.E, A = v.A, nb = (A + 63) >> 6;
  const long mstride = (long)v.n * N;
  const float* q = v.q + (long)b * N;
  float best = -INFINITY;
  int bi = INT_MAX;
  for (int j = lane; j < N; j += 64) {
    float s = q[j];
    for (int m = 1; m < E; ++m) {
      const float x = q[m * mstride + j];
      s = v.mean ? s + x : fminf(s, x);
    }
    if (v.mean) s /= (float)E;
    if (bi == INT_MAX || s > best) { best = s; bi = j; }
  }
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const float ob = __shfl_xor(best, off);
    const int oi = __shfl_xor(bi, off);
    if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
  }
  const int pick = min(__builtin_amdgcn_readfirstlane(bi), N - 1);
  best = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, best)));
  const float* src = v.actions + ((long)b * N + pick) * A;
  float w[kHeadNb];
  int cc[kHeadNb];
  bool live[kHeadNb];
#pragma unroll
  for (int j = 0; j < kHeadNb; ++j) {
    cc[j] = head_col(lane, j, A, live[j]);
    w[j] = j < nb ? src[cc[j]] : 0.f;
  }
#pragma unroll
  for (int j = 0; j < kHeadNb; ++j)
    if (j < nb && live[j]) v.action_out[(long)b * A + cc[j]] = w[j];
  if (lane == 0) {
    if (v.index) v.index[b] = pick;
    if (v.score) v.score[b] = best;
  }
}

int q_rank_wide(const QRankArgs& v, hipStream_t stream) {
  SERL_LAUNCH_CHAIN(q_rank_wide_kernel, dim3(cdiv(v.n, 4)), dim3(256), 0, stream, v);
  SERL_HIP(hipGetLastError());
  return SERL_OK;
}

// =============================================================================================
// The critic's first layer fanned out over candidates whose action block has up to 256 columns (critic_fanout_kernel's work
// split: a workgroup = one member and four observations, the base row summed once, kFanCj candidates in registers, the action
// block Wact[g] through kFanLds floats of LDS in chunks of kFanLds / D kernel rows).  The action columns are taken in blocks of
// 64: lane k of one coalesced load holds column 64 jb + k of a candidate, and the FMA loop reads value k from that register with
// v_readlane, as the narrow kernel does for its one block.  Blocks and chunks ascend, so a candidate's sum adds its action terms
// in ascending k on top of the base row: two equal candidates give equal bits wherever they stand.  With more than one block a
// chunk is staged once per register batch of candidates.  The registers are the narrow kernel's.
// =============================================================================================
template <int VPL>
__global__ __launch_bounds__(256) void critic_fanout_wide_kernel(FanoutArgs f) {
  constexpr int D = 64 * VPL, KC = kFanLds / D, CJ = kFanCj<VPL>;
  __shared__ float wl[kFanLds];
  const LnFwdArgs& a = f.l;
  const int tid = threadIdx.x, lane = tid & 63, grp = blockIdx.y, n = a.rows_per_group, N = f.N, A = f.A;
  // a wave past the last observation stages and waits with the others on the last observation's addresses and stores nothing
  const int bw = blockIdx.x * 4 + (tid >> 6);
  const bool live = bw < n;
  const int b = __builtin_amdgcn_readfirstlane(live ? bw : n - 1);
  const long pb = (long)grp * a.pstride + lane;
  float base[VPL];
  ln_gather<VPL, false>(a, (long)grp * a.S * a.slab_stride + (long)b * D + lane, pb, base);
  const float* wsrc = f.w_act + (long)grp * f.w_gstride;
  const float* arow = f.actions + (long)b * N * A;
  const int nb = (A + 63) >> 6;
  for (int j0 = 0; j0 < N; j0 += CJ) {
    float acc[CJ][VPL];
#pragma unroll
    for (int c = 0; c < CJ; ++c) {
#pragma unroll
      for (int i = 0; i < VPL; ++i) acc[c][i] = base[i];
    }
    for (int jb = 0; jb < nb; ++jb) {
      const int Ab = min(64, A - 64 * jb);   // the block's columns
      float av[CJ];
#pragma unroll
      for (int c = 0; c < CJ; ++c) {   // (a batch past the last candidate repeats the last one and is not written)
        const float x = arow[(long)min(j0 + c, N - 1) * A + 64 * jb + min(lane, Ab - 1)];
        av[c] = lane < Ab ? x : 0.f;
      }
      for (int k0 = 0; k0 < Ab; k0 += KC) {
        const int kc = min(KC, Ab - k0);
        __syncthreads();   // the rows of the chunk before are read
        for (int i = tid; i < kc * D; i += 256) wl[i] = wsrc[(long)(64 * jb + k0) * D + i];
        __syncthreads();
        for (int k = 0; k < kc; ++k) {
          float w[VPL];
#pragma unroll
          for (int i = 0; i < VPL; ++i) w[i] = wl[k * D + lane + 64 * i];
#pragma unroll
          for (int c = 0; c < CJ; ++c) {
            const float s = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, av[c]), k0 + k));
#pragma unroll
            for (int i = 0; i < VPL; ++i) acc[c][i] = fmaf(s, w[i], acc[c][i]);
          }
        }
      }
    }
    if (live) {   // (uniform over the wave)
#pragma unroll
      for (int c = 0; c < CJ; ++c)
        if (j0 + c < N) fanout_row<VPL>(a, acc[c], ((long)grp * n + b) * N + j0 + c, grp, lane, pb);
    }
  }
}

int critic_fanout_wide(const FanoutArgs& f, int D, const dim3& grid, hipStream_t stream) {
#define SERL_FAN_CASE(V) case V: SERL_LAUNCH_CHAIN(critic_fanout_wide_kernel<V>, grid, dim3(256), 0, stream, f); break;
  switch (D / 64) {
    SERL_FAN_CASE(1) SERL_FAN_CASE(2) SERL_FAN_CASE(3) SERL_FAN_CASE(4) SERL_FAN_CASE(5) SERL_FAN_CASE(6) SERL_FAN_CASE(7) SERL_FAN_CASE(8)
    SERL_FAN_CASE(9) SERL_FAN_CASE(10) SERL_FAN_CASE(11) SERL_FAN_CASE(12) SERL_FAN_CASE(13) SERL_FAN_CASE(14) SERL_FAN_CASE(15) SERL_FAN_CASE(16)
  }
#undef SERL_FAN_CASE
  SERL_HIP(hipGetLastError());
  return SERL_OK;
}
