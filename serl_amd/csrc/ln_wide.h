// The WIDE rows of an MLP layer: storage widths D, a multiple of 64 with 1024 < D <= 4096, where ONE WORKGROUP OF FOUR WAVES owns
// one row (the narrow rows of heads.hip: one wave per row, D <= 1024).  Device code and its two launchers; included once by
// heads.hip, inside namespace serl, behind the narrow rows whose helpers it shares (ln_activate, ln_dropout_n, row_dq,
// critic_loss_body, ln_for_family).  ln_fwd_multi / ln_bwd_multi hand a launch over when D > 1024.
//
// Work split.  The row is D / 64 chunks of 64 columns, 17 to 64 of them, dealt to the four waves in turn: chunk c belongs to wave
// c & 3, so wave w holds chunks w, w + 4, w + 8, ... and lane l of it the columns 64 (w + 4 j) + l -- the strided layout of the
// narrow rows: every load and store instruction of a wave covers 256 consecutive bytes.  CPW = ceil(D / 256), 5 to 16, is the
// template parameter: the chunks of the wave that holds most, hence a lane's columns and the register footprint -- at most the
// 16 of the narrow row at 1024, which fits the chain's budget beside two trunk workgroups.  17 chunks are dealt
// 5 / 4 / 4 / 4.  Chunks j < CPW - 1 exist in every wave (4 (CPW - 1) < D / 64); the TAIL chunk j = CPW - 1 exists in wave w when
// w + 4 (CPW - 1) < D / 64 and is predicated by DESIGN.md section 8's rule: the address is clamped (to the wave's chunk 0), the load is
// unconditional, the value is selected to 0 afterwards and the store is skipped.  No lane reads or writes outside its row.
//
// Exchange.  A row sum is a lane's columns in ascending order, then the xor butterfly of the wave (wave_sum2), then 4 x k floats
// through LDS behind ONE barrier, added by every wave in wave order 0, 1, 2, 3: the bits of a row depend on D alone, not on the
// schedule, the grid or where the row stands.  Every reduction of a kernel has LDS words of its own, so none waits for the
// one before to be read: the forward LayerNorm row exchanges (s1, s2) and the Q-head rider its dot; the backward row its two row
// sums; the plain rows the rider alone.  12 floats of LDS forward; the backward kernels exchange inside the 4 KB their
// critic-loss rider workgroup reduces in (the narrow backward kernels hold the same 4 KB).
//
// Forms: LayerNorm and plain (LN), ragged by a.d (the statistics divide by the true width, the pads stay exactly 0 -- a.d is read
// at run time: a row of D live columns divides by D through the same instruction), tanh / relu / swish, xhat / rstd / the plain
// pre-activation as the backward reads them, ln_gather's arithmetic per column (bias first, then the slabs in index order),
// dy as a tensor, as the rank-1 dq (x) w and as dq_inline beside the critic-loss rider.
// Dropout (the DROP instantiations, launched when an instance of the launch carries a mask; every other launch runs the kernels it
// always ran): a wave applies the keep decisions to the chunks it was dealt BEFORE the row sums go through LDS -- the forward row to
// the gathered Dense output, the backward rows to dx, stating the forward's decision again.  Element (row r, true column c) is
// decision r * Nt + c, Nt = a.d or D (ln_dropout_n of heads.hip); the tail chunk's and the pads' addresses are clamped, the load
// is unconditional and the value selected afterwards.  A decision depends on (r, c) alone and the exchange is unchanged: a row's
// bits still depend on D alone.  The key's decisions are taken in column order in a loop that is not unrolled.
// The kernels are built without packed fp32 instructions (v_pk_*_f32).
#pragma once

#if defined(__HIP_DEVICE_COMPILE__)   // (a target feature of the device pass alone)
#define SERL_WIDE_KERNEL __attribute__((target("no-packed-fp32-ops"))) __global__ __launch_bounds__(256)
#else
#define SERL_WIDE_KERNEL __global__ __launch_bounds__(256)
#endif

constexpr int kWideMax = 4096;   // the widest row: 64 chunks, 16 per wave

// a lane's column j: 64 (wave + 4 j) + lane; the tail chunk of a wave that has none is clamped to the wave's chunk 0
template <int CPW>
__device__ __forceinline__ int wide_col(int j, int c0, bool tail_ok) { return (j < CPW - 1 || tail_ok) ? c0 + 256 * j : c0; }

// s1 and s2 of the four waves' lanes summed, the sums left in every lane: butterfly, 8 floats of LDS at x, one barrier, wave order
__device__ __forceinline__ void wide_sum2(float& s1, float& s2, float* x, int wave, int lane) {
  wave_sum2(s1, s2);
  if (lane == 0) { x[2 * wave] = s1; x[2 * wave + 1] = s2; }
  __syncthreads();
  s1 = ((x[0] + x[2]) + x[4]) + x[6];
  s2 = ((x[1] + x[3]) + x[5]) + x[7];
}

// Dropout on a lane's CPW values of local row `lrow`: ln_dropout_n (heads.hip) in the wide column map -- wide_col's columns; the
// tail of a wave that has no tail chunk is not live
template <int CPW>
__device__ __forceinline__ void wide_dropout(const LnDrop& d, long lrow, int c0, bool tail_ok, int Nt, float (&v)[CPW]) {
  ln_dropout_n(d, lrow, Nt, v, [&](int j) SERL_LAMBDA_INLINE { return wide_col<CPW>(j, c0, tail_ok); },
               [&](int j) SERL_LAMBDA_INLINE { return (j < CPW - 1 || tail_ok) && c0 + 256 * j < Nt; });
}

// The forward row (ln_row / plain_row of heads.hip at these widths).  x: 12 floats of LDS.  DROP: see above.
template <int CPW, bool LN, bool DROP>
__device__ __forceinline__ void wide_row(const LnFwdArgs& a, int D, int row, int wave, int lane, float* x) {
  const bool tail_ok = wave + 4 * (CPW - 1) < (D >> 6);
  const int c0 = 64 * wave + lane;
  const int grp = row / a.rows_per_group;
  const long lrow = row - grp * a.rows_per_group;
  const long base = (long)grp * a.S * a.slab_stride + lrow * D;
  const long pb = (long)grp * a.pstride;
  float v[CPW];
#pragma unroll
  for (int j = 0; j < CPW; ++j) v[j] = a.bias ? a.bias[pb + wide_col<CPW>(j, c0, tail_ok)] : 0.f;
#pragma unroll 2
  for (int s = 0; s < a.S; ++s) {
    const long o = base + (long)s * a.slab_stride;
#pragma unroll
    for (int j = 0; j < CPW; ++j) v[j] += a.slabs[o + wide_col<CPW>(j, c0, tail_ok)];
  }
  v[CPW - 1] = tail_ok ? v[CPW - 1] : 0.f;
  if constexpr (DROP) {
    if (a.drop.mode != kLnDropNone) wide_dropout<CPW>(a.drop, lrow, c0, tail_ok, a.d ? a.d : D, v);   // (uniform: the launch's instance)
  }
  float rstd = 0.f;
  if constexpr (LN) {
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < CPW; ++j) { s1 += v[j]; s2 += v[j] * v[j]; }
    wide_sum2(s1, s2, x, wave, lane);
    float mean;
    ln_mean_rstd_n(s1, s2, a.d ? a.d : D, mean, rstd);
#pragma unroll
    for (int j = 0; j < CPW; ++j) {   // v: the row's values, then its pre-activations, then y
      const int col = wide_col<CPW>(j, c0, tail_ok);
      float xh = (v[j] - mean) * rstd;
      if constexpr (DROP) xh = col < (a.d ? a.d : D) ? xh : 0.f;   // (xhat is kept 0 in a ragged row's pads)
      v[j] = xh * a.gamma[pb + col] + a.beta[pb + col];
      if (a.xhat && (j < CPW - 1 || tail_ok)) a.xhat[(long)row * D + col] = xh;
    }
  } else if (a.xhat) {   // a plain layer keeps its pre-activation where a LayerNorm layer keeps xhat
#pragma unroll
    for (int j = 0; j < CPW; ++j)
      if (j < CPW - 1 || tail_ok) a.xhat[(long)row * D + wide_col<CPW>(j, c0, tail_ok)] = v[j];
  }
  ln_activate(a.act, v);
  float d = 0.f;
#pragma unroll
  for (int j = 0; j < CPW; ++j) {
    const int col = wide_col<CPW>(j, c0, tail_ok);
    const bool ok = j < CPW - 1 || tail_ok;
    if (ok) a.y[lrow * a.ld_y + (long)grp * a.y_goff + col] = v[j];
    if (a.dot_out) {
      const float t = v[j] * a.dot_w[(long)grp * a.dot_gstride + col];
      d += ok ? t : 0.f;
    }
  }
  if (LN && a.rstd && threadIdx.x == 0) a.rstd[row] = rstd;
  if (a.dot_out) {   // (uniform over the launch's instance: every wave meets the barrier)
    float unused = 0.f;
    wave_sum2(d, unused);
    if (lane == 0) x[8 + wave] = d;
    __syncthreads();
    d = ((x[8] + x[9]) + x[10]) + x[11];
    if (threadIdx.x == 0) a.dot_out[row] = d + a.dot_b[(long)grp * a.dot_b_gstride];
  }
}

// LN: LayerNorm or plain rows; DROP: a launch in which an instance has Dropout
template <int CPW, bool LN, bool DROP>
SERL_WIDE_KERNEL void ln_wide_fwd_kernel(Multi<LnFwdArgs> mv, int D) {
  __shared__ float x[12];
  const LnFwdArgs& a = mv.v[blockIdx.y];   // blockIdx.y = instance, blockIdx.x = row
  if ((int)blockIdx.x >= a.rows) return;   // (the whole workgroup)
  wide_row<CPW, LN, DROP>(a, D, blockIdx.x, threadIdx.x >> 6, threadIdx.x & 63, x);
}

// The backward LayerNorm row (ln_bwd_row of heads.hip at these widths; ragged by a.d).  x: 8 floats of LDS.  DROP: dx wrt the
// LayerNorm's input, then wrt the Dense output in front of the Dropout.
template <int CPW, bool DROP = false>
__device__ __forceinline__ void wide_bwd_row(const LnBwdArgs& a, const LossArgs& L, int row, int wave, int lane, float* x) {
  const int D = a.D, live = a.d ? a.d : D;
  const bool tail_ok = wave + 4 * (CPW - 1) < (D >> 6);
  const int c0 = 64 * wave + lane;
  const int grp = row / a.rows_per_group;
  const long lr = row - grp * a.rows_per_group;
  const long pb = (long)grp * a.pstride;
  const float dqr = row_dq(a, L, row, lr);
  float dg[CPW], dxh[CPW], xh[CPW], y[CPW], gam[CPW];
#pragma unroll
  for (int j = 0; j < CPW; ++j) {
    const int col = wide_col<CPW>(j, c0, tail_ok);
    y[j] = a.y[lr * a.ld_y + (long)grp * a.y_goff + col];
    dg[j] = a.dq_w ? dqr * a.dq_w[(long)grp * a.dq_w_gstride + col] : a.dy[lr * a.ld_dy + (long)grp * a.dy_goff + col];
    xh[j] = a.xhat[(long)row * D + col];
    gam[j] = a.gamma[pb + col];
  }
  if (a.act == kActTanh) {
#pragma unroll
    for (int j = 0; j < CPW; ++j) dg[j] *= 1.f - y[j] * y[j];
  } else if (a.act == kActRelu) {
#pragma unroll
    for (int j = 0; j < CPW; ++j) dg[j] = y[j] > 0.f ? dg[j] : 0.f;
  } else {   // swish: sigma(p) + y (1 - sigma(p)) with p = gamma xhat + beta recomputed
#pragma unroll
    for (int j = 0; j < CPW; ++j) {
      const float sg = sigmoid_stable(xh[j] * gam[j] + a.beta[pb + wide_col<CPW>(j, c0, tail_ok)]);
      dg[j] *= sg + y[j] * (1.f - sg);
    }
  }
  dg[CPW - 1] = tail_ok ? dg[CPW - 1] : 0.f;
  xh[CPW - 1] = tail_ok ? xh[CPW - 1] : 0.f;
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int j = 0; j < CPW; ++j) {
    dxh[j] = dg[j] * gam[j];
    s1 += dxh[j];
    s2 += dxh[j] * xh[j];
  }
  wide_sum2(s1, s2, x, wave, lane);
  const float inv = 1.0f / (float)live, m1 = s1 * inv, m2 = s2 * inv;
  const float rstd = a.rstd[row];
  if constexpr (DROP) {
#pragma unroll
    for (int j = 0; j < CPW; ++j) dxh[j] = rstd * (dxh[j] - m1 - xh[j] * m2);
    if (a.drop.mode != kLnDropNone) wide_dropout<CPW>(a.drop, lr, c0, tail_ok, live, dxh);
#pragma unroll
    for (int j = 0; j < CPW; ++j) {
      const int col = wide_col<CPW>(j, c0, tail_ok);
      if (j < CPW - 1 || tail_ok) {
        a.dx[(long)row * D + col] = col < live ? dxh[j] : 0.f;
        a.dg[(long)row * D + col] = dg[j];
      }
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < CPW; ++j) {
    const int col = wide_col<CPW>(j, c0, tail_ok);
    if (j < CPW - 1 || tail_ok) {
      a.dx[(long)row * D + col] = col < live ? rstd * (dxh[j] - m1 - xh[j] * m2) : 0.f;   // (a ragged row: dx is 0 in the pads)
      a.dg[(long)row * D + col] = dg[j];
    }
  }
}

// The backward plain row (plain_bwd_row of heads.hip at these widths): no statistics, no exchange; dx alone is written.
template <int CPW, bool DROP = false>
__device__ __forceinline__ void wide_plain_bwd_row(const LnBwdArgs& a, const LossArgs& L, int row, int wave, int lane) {
  const int D = a.D;
  const bool tail_ok = wave + 4 * (CPW - 1) < (D >> 6);
  const int c0 = 64 * wave + lane;
  const int grp = row / a.rows_per_group;
  const long lr = row - grp * a.rows_per_group;
  const float dqr = row_dq(a, L, row, lr);
  float dg[CPW], y[CPW];
#pragma unroll
  for (int j = 0; j < CPW; ++j) {
    const int col = wide_col<CPW>(j, c0, tail_ok);
    y[j] = a.y[lr * a.ld_y + (long)grp * a.y_goff + col];
    dg[j] = a.dq_w ? dqr * a.dq_w[(long)grp * a.dq_w_gstride + col] : a.dy[lr * a.ld_dy + (long)grp * a.dy_goff + col];
  }
  if (a.act == kActTanh) {
#pragma unroll
    for (int j = 0; j < CPW; ++j) dg[j] *= 1.f - y[j] * y[j];
  } else if (a.act == kActRelu) {
#pragma unroll
    for (int j = 0; j < CPW; ++j) dg[j] = y[j] > 0.f ? dg[j] : 0.f;
  } else {   // swish from the pre-activation the forward row kept in xhat
#pragma unroll
    for (int j = 0; j < CPW; ++j) {
      const float sg = sigmoid_stable(a.xhat[(long)row * D + wide_col<CPW>(j, c0, tail_ok)]);
      dg[j] *= sg + y[j] * (1.f - sg);
    }
  }
  if constexpr (DROP) {
    if (a.drop.mode != kLnDropNone) wide_dropout<CPW>(a.drop, lr, c0, tail_ok, a.d ? a.d : D, dg);
  }
#pragma unroll
  for (int j = 0; j < CPW; ++j)
    if (j < CPW - 1 || tail_ok) a.dx[(long)row * D + wide_col<CPW>(j, c0, tail_ok)] = dg[j];
}

// blockIdx.y = instance, blockIdx.x = row; the LAST workgroup of instance 0 is the critic-loss rider when loss.on, as in the
// narrow launches.  LN, DROP: as in ln_wide_fwd_kernel.
template <int CPW, bool LN, bool DROP>
SERL_WIDE_KERNEL void ln_wide_bwd_kernel(Multi<LnBwdArgs> mv, LossArgs loss) {
  __shared__ float red[4][256];
  if (loss.on && blockIdx.y == 0 && blockIdx.x == gridDim.x - 1) { critic_loss_body(loss, red); return; }
  const LnBwdArgs& a = mv.v[blockIdx.y];
  if ((int)blockIdx.x >= a.rows) return;   // (the whole workgroup)
  if constexpr (LN) wide_bwd_row<CPW, DROP>(a, loss, blockIdx.x, threadIdx.x >> 6, threadIdx.x & 63, &red[0][0]);
  else wide_plain_bwd_row<CPW, DROP>(a, loss, blockIdx.x, threadIdx.x >> 6, threadIdx.x & 63);
}

// wide width -> launch(CPW), CPW = ceil(D / 256); the family comes from ln_for_family (heads.hip), whose RAGGED these rows do not
// read: they are ragged by a.d at run time
template <class F>
static int wide_for_width(int D, F&& launch) {
  switch (cdiv(D / 64, 4)) {
#define SERL_WIDE_CASE(V) case V: launch(IntC<V>{}); break;
    SERL_WIDE_CASE(5) SERL_WIDE_CASE(6) SERL_WIDE_CASE(7) SERL_WIDE_CASE(8) SERL_WIDE_CASE(9) SERL_WIDE_CASE(10)
    SERL_WIDE_CASE(11) SERL_WIDE_CASE(12) SERL_WIDE_CASE(13) SERL_WIDE_CASE(14) SERL_WIDE_CASE(15) SERL_WIDE_CASE(16)
#undef SERL_WIDE_CASE
    default: serl::set_error("wide LayerNorm width %d has no kernel", D); return SERL_ERR_INVALID;
  }
  return SERL_OK;
}

// mv, rows (the most of any instance), D, plain, drop (an instance carries Dropout) as ln_fwd_multi validated them; one workgroup
// per row and instance
int ln_wide_fwd(const Multi<LnFwdArgs>& mv, int n, int rows, int D, bool plain, bool drop, hipStream_t stream) {
  SERL_REQUIRE(D > 1024 && D <= kWideMax && D % 64 == 0 && rows >= 1, "wide LayerNorm row: width %d, %d rows", D, rows);
  const dim3 grid(rows, n);
  const int rc = ln_for_family(plain, false, drop, [&](auto ln, auto, auto dr) {
    return wide_for_width(D, [&](auto cpw) {
      SERL_LAUNCH_CHAIN((ln_wide_fwd_kernel<SERL_C(cpw), SERL_C(ln), SERL_C(dr)>), grid, dim3(256), 0, stream, mv, D);
    });
  });
  if (rc != SERL_OK) return rc;
  SERL_HIP(hipGetLastError());
  return SERL_OK;
}

// ... as ln_bwd_multi validated them (every instance D wide); the rider workgroup behind the rows when loss.on
int ln_wide_bwd(const Multi<LnBwdArgs>& mv, int n, int rows, int D, bool plain, bool drop, const LossArgs& loss, hipStream_t stream) {
  SERL_REQUIRE(D > 1024 && D <= kWideMax && D % 64 == 0 && rows >= 1, "wide LayerNorm backward: width %d, %d rows", D, rows);
  const dim3 grid(rows + (loss.on ? 1 : 0), n);
  const int rc = ln_for_family(plain, false, drop, [&](auto ln, auto, auto dr) {
    return wide_for_width(D, [&](auto cpw) {
      SERL_LAUNCH_CHAIN((ln_wide_bwd_kernel<SERL_C(cpw), SERL_C(ln), SERL_C(dr)>), grid, dim3(256), 0, stream, mv, loss);
    });
  });
  if (rc != SERL_OK) return rc;
  SERL_HIP(hipGetLastError());
  return SERL_OK;
}
