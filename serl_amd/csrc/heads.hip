// Dense building blocks of the SAC/DrQ update on MI355X: strided/batched/split-K fp32 MFMA GEMM and
// the fused elementwise/normalisation kernels around it (LayerNorm+tanh forward/backward,
// SpatialLearnedEmbeddings, tanh-Gaussian policy head, REDQ target, losses, 3x Adam + target EMA).
// Reference semantics are cited per kernel (paths relative to serl_launcher/serl_launcher/).
#include <algorithm>
#include <cstdlib>

#include "heads.h"
#include "jaxrng.h"
#include "ln_stats.h"
#include "prof.h"

namespace serl {

// every kernel launch of the update chain is counted (serl_debug_chain_launches: the tests pin the chain's launch count)
long g_chain_launches = 0;
#define SERL_LAUNCH_CHAIN(...) do { ++g_chain_launches; hipLaunchKernelGGL(__VA_ARGS__); } while (0)

typedef float f32x16 __attribute__((ext_vector_type(16)));

// =============================================================================================
// GEMM  C[z] = A[b] * B[b] over K-split `s`   (z = b*splitk + s)
// 64x64 tile per 256-thread workgroup (2x2 waves, one 32x32 fp32-MFMA tile each), BK = 32.
// The update chain runs beside the frozen trunk of the next batch, whose conv workgroups own nearly the
// whole register file and LDS of every CU; a chain kernel starts only in the space a retiring conv
// workgroup frees.  The kernel is therefore built lean -- ~60 VGPRs, 18 KB LDS (single-buffered, next chunk
// prefetched in registers) -- so that several of its workgroups fit into one freed conv slot.
// Operands are read with 16-byte vectors along whichever dimension is contiguous (transposes are free:
// A may be k- or m-contiguous, B k- or n-contiguous).  A k-contiguous operand is stored [row][k] with a
// 36-float pitch, so one conflict-free ds_read_b128 feeds four MFMAs: inside each block of 8 k's, lanes 0-31
// take k = 0..3 and lanes 32-63 k = 4..7 (the K order of a sum is free).  A row-contiguous operand keeps its
// orientation in LDS, [k][row] with a 68-float pitch: its 16-byte global vectors become single conflict-free
// ds_write_b128 and a fragment is four conflict-free ds_read_b32 (consecutive lanes = consecutive rows).  Round 2
// transposed such operands on the way into LDS with scalar stores at a 36-float row pitch: 8 lanes per bank,
// SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.62 for gemm_f32_kernel<true, false> (profiles/r02_mfma_counters.json).
// Edges are zero-filled; slabs are summed by the consumer (reduce_slabs / ln_fwd_kernel), which keeps the
// K-split deterministic.  Arbitrary element strides fall back to gemm_f32_strided_kernel.
// =============================================================================================
constexpr int kGBM = 64, kGBN = 64, kGBK = 32, kGP = 36, kGPT = 68;
constexpr int kGTile = kGBM * kGP;   // floats per operand tile in LDS (>= kGBK * kGPT)
static_assert(kGBK * kGPT <= kGTile, "the [k][row] layout must fit the tile");
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));  // global loads need only 4-byte alignment

// 4 consecutive floats at p of which the first `valid` exist (<= 0: none, >= 4: all); missing ones are 0
__device__ __forceinline__ f32x4 ld4(const float* p, int valid) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (valid >= 4) {
    v = *reinterpret_cast<const f32x4u*>(p);
  } else if (valid > 0) {
    v[0] = p[0];
    if (valid > 1) v[1] = p[1];
    if (valid > 2) v[2] = p[2];
  }
  return v;
}

// One operand tile X[r0 .. r0+64)[k0 .. k0+32) with element strides (sR, sK), one of which is 1.
// KFAST: vectors run along k (thread -> row idx>>3, k 4*(idx&7)); otherwise along the rows
// (thread -> k idx>>4, rows 4*(idx&15)) and are transposed on the way into LDS.
template <bool KFAST>
struct OperandLoader {
  const float* p[2];
  int lim[2];   // KFAST: row valid ? 1 : 0      else: number of valid rows from this thread's first row
  int kofs[2];  // k offset of this thread's vector inside the chunk
  long step;    // pointer advance per chunk
  __device__ __forceinline__ void init(const float* X, long sR, long sK, int r0, int R, int k_begin, int tid) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = tid + 256 * i;
      if (KFAST) {
        const int r = idx >> 3;
        kofs[i] = 4 * (idx & 7);
        lim[i] = (r0 + r < R) ? 1 : 0;
        p[i] = X + (long)(r0 + r) * sR + (k_begin + kofs[i]);
      } else {
        const int rq = 4 * (idx & 15);
        kofs[i] = idx >> 4;
        lim[i] = R - (r0 + rq);
        p[i] = X + (long)(k_begin + kofs[i]) * sK + (r0 + rq);
      }
    }
    step = KFAST ? kGBK : kGBK * sK;
  }
  // loads the chunk starting at k0 (elements at k >= k_end are zero) and advances to the next chunk
  __device__ __forceinline__ void load(f32x4 (&r)[2], int k0, int k_end) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int krem = k_end - (k0 + kofs[i]);
      const int valid = KFAST ? (lim[i] ? krem : 0) : (krem > 0 ? lim[i] : 0);
      r[i] = ld4(p[i], valid);
      p[i] += step;
    }
  }
  __device__ __forceinline__ void store(float* S, const f32x4 (&r)[2], int tid) const {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = tid + 256 * i;
      if (KFAST) *reinterpret_cast<f32x4*>(S + (idx >> 3) * kGP + 4 * (idx & 7)) = r[i];      // [row][k]
      else *reinterpret_cast<f32x4*>(S + (idx >> 4) * kGPT + 4 * (idx & 15)) = r[i];          // [k][row]
    }
  }
  // the four operand values of this lane for k = 8q + 4*lh + (0..3) of tile row `row`
  __device__ __forceinline__ static f32x4 frag(const float* S, int row, int lh, int q) {
    if (KFAST) return *reinterpret_cast<const f32x4*>(S + row * kGP + 8 * q + 4 * lh);
    const float* p = S + (8 * q + 4 * lh) * kGPT + row;
    return (f32x4){p[0], p[kGPT], p[2 * kGPT], p[3 * kGPT]};
  }
};

// =============================================================================================
// Last-arriver epilogues (GemmDesc::epi).  The update chain is ~60 small dependent kernels; a launch boundary costs it more
// than most of these kernels do.  Where a GEMM was followed by a kernel whose only job was to sum the GEMM's slabs (K-split
// or ensemble members) and apply something row-local (bias + LayerNorm + tanh, the tanh-Gaussian head), the consumer now runs
// inside the GEMM launch, in the workgroup that arrives LAST at the output tile:
//   * every workgroup writes its 64x64 slab tile with 16-byte WRITE-THROUGH stores (buffer_store_dwordx4 sc1: the bytes leave
//     the XCD's L2, so no release fence / L2 write-back is needed), every wave drains its stores (s_waitcnt vmcnt(0), written
//     as inline asm so the compiler cannot drop it), __syncthreads, then ONE lane takes a ticket from the tile's arrival
//     counter with a returning memory-side atomic;
//   * the workgroup that draws the last ticket re-zeroes the counter and reads every slab of the tile with sc1 loads (served
//     past its own L1: no acquire fence / invalidate needed) IN INDEX ORDER -- the same order the separate reduce_slabs /
//     ln_fwd kernels summed in, so fused and un-fused results are bit-identical (tests assert exact equality).
// This is the "in-launch split-K reduction" recipe of cdna_hip_programming.md (sc1 stores + drain + barrier + relaxed
// ticket; sc1 loads on the reducer): correct for any placement of a tile's workgroups over CUs / XCDs, no spinning (nobody
// waits for anybody), no cache maintenance next to the co-running trunk pass.  The MFMA accumulator layout gives a lane one
// COLUMN of 16 rows; the tile is turned into row-major 16-byte vectors through the (now idle) operand LDS, 16 rows per wave
// and pass.  Slab images are padded scratch (ldc % 64 == 0, whole tiles): no edge handling on the slab side.
// =============================================================================================
constexpr int kEpiPitch = 36;                       // floats per LDS row of the transpose scratch
constexpr int kEpiScratch = 4 * 16 * kEpiPitch;     // floats (4 waves x 16 rows); one more int behind it = the "I am last" flag
constexpr int kSc1 = 16;                            // buffer aux bits: sc1 (write-through store / L1-bypassing load)
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc_of(const void* p) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, 0x7fffffff, 0x00020000);
}
__device__ __forceinline__ f32x4 ld_sc1(__amdgpu_buffer_rsrc_t r, long float_off) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)(float_off * 4), 0, kSc1));
}
__device__ __forceinline__ float ld1_sc1(__amdgpu_buffer_rsrc_t r, long float_off) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)(float_off * 4), 0, kSc1));
}

// accumulators of wave (wm, wn) -> slab tile rows m0 + wm*32 .., columns n0 + wn*32 .. as 16-byte sc1 stores
__device__ __forceinline__ void store_tile_sc1(float* C, long ldc, int m0, int n0, const f32x16& acc, float* scratch, int tid) {
  const int lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1, li = lane & 31, lh = lane >> 5;
  float* S = scratch + wave * 16 * kEpiPitch;
  const __amdgpu_buffer_rsrc_t rs = rsrc_of(C);
#pragma unroll
  for (int p = 0; p < 2; ++p) {
#pragma unroll
    for (int r = 8 * p; r < 8 * p + 8; ++r) S[(8 * ((r >> 2) & 1) + 4 * lh + (r & 3)) * kEpiPitch + li] = acc[r];
    __builtin_amdgcn_wave_barrier();   // (wave-private scratch: LDS ops of one wave execute in order)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = (lane >> 3) + 8 * h, c4 = lane & 7;
      const f32x4 v = *reinterpret_cast<const f32x4*>(S + row * kEpiPitch + 4 * c4);
      const long off = (long)(m0 + wm * 32 + 16 * p + row) * ldc + n0 + wn * 32 + 4 * c4;
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, v), rs, (int)(off * 4), 0, kSc1);
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// every wave has drained its sc1 stores -> one ticket; true in the workgroup that arrived last (which re-zeroes the counter)
__device__ __forceinline__ bool arrive_is_last(int* ctr, int total, int* lds_flag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const int old = __hip_atomic_fetch_add(ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    const int last = old == total - 1;
    if (last) __hip_atomic_store(ctr, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    *lds_flag = last;
  }
  __syncthreads();
  return *lds_flag != 0;
}

__device__ __forceinline__ float softplusf(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ uint64_t mix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
// N(0,1) draw number i of stream `seed` (the element's position in the GLOBAL tensor: the same for whichever rank owns it)
__device__ __forceinline__ float hash_normal(uint64_t seed, uint64_t i) {
  const uint64_t r = mix64(seed ^ mix64(i));
  const float u1 = ((float)(uint32_t)(r >> 40) + 1.0f) * (1.0f / 16777217.0f);
  const float u2 = (float)(uint32_t)((r >> 8) & 0xFFFFFF) * (1.0f / 16777216.0f);
  return sqrtf(-2.f * logf(u1)) * cosf(6.283185307179586f * u2);
}

// The activation of a LayerNorm row, and what multiplies dy in its backward (mlp.py:19-31).  `act` (kAct*) is a field of the launch's
// instance, so the branch is uniform over the wave -- a scalar compare and branch, no exec masking (no lane takes another way) --
// and the rows take it ONCE, over all the columns a lane holds: the tanh path then runs the instructions it always ran.
// swish(p) = p * sigmoid(p) with sigmoid from e = exp(-|p|) in (0, 1]: 1 / (1 + e) for p >= 0, e / (1 + e) below.  No exponent
// overflows and nothing is NaN at any finite p; at p -> -inf both e and swish go to -0.  Two quarter-rate instructions per
// element (v_exp_f32, v_rcp_f32; 1 ulp each), fewer than tanhf spends.
__device__ __forceinline__ float sigmoid_stable(float p) {
  const float e = __expf(-fabsf(p));
  const float r = __builtin_amdgcn_rcpf(1.f + e);
  return p >= 0.f ? r : e * r;
}
template <int N>
__device__ __forceinline__ void ln_activate(int act, float (&v)[N]) {   // in place: pre-activations -> y
  if (act == kActTanh) {
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = tanhf(v[j]);
  } else if (act == kActRelu) {
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = fmaxf(v[j], 0.f);
  } else {
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] *= sigmoid_stable(v[j]);
  }
}
// dg[j] = dy[j] * act'(pre[j]) in place (dg holds dy on entry).  tanh: 1 - y^2.  ReLU: y > 0 -- the gradient AT 0 is 0, as
// jax.nn.relu's.  swish: sigma(p) + y (1 - sigma(p)) with p = gam * xh + beta recomputed (pbeta: the lane's first beta, its
// columns BSTRIDE floats apart: beta + boff; beta is nullptr on the other paths, so the pointer is formed on this one alone).
template <int N, int BSTRIDE>
__device__ __forceinline__ void ln_act_grad(int act, float (&dg)[N], const float (&y)[N], const float (&xh)[N], const float (&gam)[N],
                                            const float* beta, long boff) {
  if (act == kActTanh) {
#pragma unroll
    for (int j = 0; j < N; ++j) dg[j] *= 1.f - y[j] * y[j];
  } else if (act == kActRelu) {
#pragma unroll
    for (int j = 0; j < N; ++j) dg[j] = y[j] > 0.f ? dg[j] : 0.f;
  } else {
    const float* pbeta = beta + boff;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const float sg = sigmoid_stable(xh[j] * gam[j] + pbeta[j * BSTRIDE]);
      dg[j] *= sg + y[j] * (1.f - sg);
    }
  }
}

// LayerNorm(eps 1e-6, fast variance) + activation of ONE row of width D = 64 * VPL by one wave (mlp.py:24-31,
// resnet_v1.py:371-374, encoding.py:66-68): a lane holds VPL of the row's columns, 64 .. 1024 columns in all.
//   pre = bias[g] + sum_s slab[s][row] (slabs read in index order);  y = act(gamma[g]*xhat + beta[g])  (act: LnFwdArgs::act)
// Lane-to-column layout.  STRIDED: lane l holds columns l, l + 64, ..., l + 64 (VPL - 1); every load / store instruction of the
// wave then covers 64 consecutive floats (256 bytes, two whole cache lines) whatever VPL is.  BLOCKED (width 256 alone, VPL == 4):
// lane l holds columns 4 l .. 4 l + 3, its bias and slab values one 16-byte access each; a block of 12 or 20 bytes (VPL = 3 or 5)
// has no such access, and a 4-byte access per column would stride the wave over the row.  (Multiples of 256 could take 16-byte
// accesses in a blocked-by-256 layout; the strided layout serves every other width until one of them has a speed target.)
// Same arithmetic in both: bias, then the slabs in index order; a lane sums its columns in ascending order, then the xor
// butterfly.  Fused and one-per-operation schedules compare bit for bit (tests assert exact equality).
// A lane's column j is ln_col0(lane) + kLnStep * j.
template <int VPL, bool BLOCKED>
__device__ __forceinline__ int ln_col0(int lane) { return BLOCKED ? lane * VPL : lane; }
template <bool BLOCKED>
constexpr int kLnStep = BLOCKED ? 1 : 64;
// The row's values in a lane: v[j] = bias[pb + kLnStep j] (0 without a bias) + sum_s slabs[base + s slab_stride + kLnStep j], the
// slabs added in index order.  A blocked lane asks for its 16 bytes as such -- the compiler cannot prove their alignment and
// would not merge four scalar loads -- and keeps four slab reads in flight (unrolled by hand: the compiler's own unrolling by 4
// takes 6 VGPRs more); a strided lane keeps 2 VPL reads in flight.
template <int VPL, bool BLOCKED>
__device__ __forceinline__ void ln_gather(const LnFwdArgs& a, long base, long pb, float (&v)[VPL]) {
  if constexpr (BLOCKED) {
    static_assert(VPL == 4, "the blocked layout is one 16-byte access per lane");
    auto slab = [&](int s) { return *reinterpret_cast<const f32x4*>(a.slabs + base + (long)s * a.slab_stride); };
    f32x4 acc = a.bias ? *reinterpret_cast<const f32x4*>(a.bias + pb) : (f32x4){0.f, 0.f, 0.f, 0.f};
    int s = 0;
    for (; s + 4 <= a.S; s += 4) {
      const f32x4 x0 = slab(s), x1 = slab(s + 1), x2 = slab(s + 2), x3 = slab(s + 3);
      acc += x0; acc += x1; acc += x2; acc += x3;
    }
    for (; s < a.S; ++s) acc += slab(s);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = acc[j];
  } else {
#pragma unroll
    for (int j = 0; j < VPL; ++j) v[j] = a.bias ? a.bias[pb + 64 * j] : 0.f;
#pragma unroll 2
    for (int s = 0; s < a.S; ++s) {
      const long o = base + (long)s * a.slab_stride;
#pragma unroll
      for (int j = 0; j < VPL; ++j) v[j] += a.slabs[o + 64 * j];
    }
  }
}
// Dropout on a lane's VPL values of local row `lrow` (LnDrop, internal.h; mlp.py:27-28): kept elements are divided by keep as
// flax does (inputs / keep_prob), dropped ones are exactly 0.  The forward row applies it to the gathered Dense output, the
// backward row to dx; both state the element's index as (row0 + lrow) * D + column, whatever the lane layout.  Called under a
// wave-uniform branch on d.mode != kLnDropNone; the mode is uniform too.
template <int VPL, bool BLOCKED>
__device__ __forceinline__ void ln_dropout(const LnDrop& d, long lrow, int c0, float (&v)[VPL]) {
  constexpr int D = 64 * VPL, kStep = kLnStep<BLOCKED>;
  const uint32_t thr = (uint32_t)(d.keep * 16777216.f);
#pragma unroll
  for (int j = 0; j < VPL; ++j) {
    const int col = c0 + kStep * j;
    bool keep;
    if (d.mode == kLnDropMask) {
      keep = d.mask[lrow * D + col] != 0;
    } else {
      const uint64_t e = (uint64_t)(d.row0 + lrow) * (uint64_t)D + (uint64_t)col;
      if (d.mode == kLnDropKey) keep = bits_to_unit(random_bits_at(d.key[0], d.key[1], (uint64_t)d.total_rows * (uint64_t)D, e)) < d.keep;
      else keep = (uint32_t)(mix64(d.seed ^ mix64(e)) & 0xFFFFFFull) < thr;
    }
    v[j] = keep ? v[j] / d.keep : 0.f;
  }
}
// Returns the fused row-dot (dot_out's value, in every lane; 0 without one).
// DROP: the instantiation of the launches that carry an instance with Dropout (ln_fwd_drop_kernel); the rows of every other launch
// are the DROP = false instantiation, whose text -- and therefore whose contraction into fused multiply-adds -- is what it was.
// RAGGED: the instantiation of a zero-padded row of true width a.d < D (heads.h): the statistics divide by a.d.  Nothing else
// differs: the pads of the bias and of the slabs are 0 and add nothing to the sums, and gamma == beta == 0 there gives y == act(0) == 0.
template <int VPL, bool BLOCKED, bool DROP = false, bool RAGGED = false>
__device__ __forceinline__ float ln_row(const LnFwdArgs& a, int row, int lane) {
  constexpr int D = 64 * VPL, kStep = kLnStep<BLOCKED>;
  const int grp = row / a.rows_per_group;
  const long lrow = row - grp * a.rows_per_group;
  const int c0 = ln_col0<VPL, BLOCKED>(lane);
  const long base = (long)grp * a.S * a.slab_stride + lrow * D + c0;
  const long pb = (long)grp * a.pstride + c0;
  float v[VPL];
  ln_gather<VPL, BLOCKED>(a, base, pb, v);
  if constexpr (DROP) {
    if (a.drop.mode != kLnDropNone) ln_dropout<VPL, BLOCKED>(a.drop, lrow, c0, v);   // (uniform: the launch's instance)
  }
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int j = 0; j < VPL; ++j) { s1 += v[j]; s2 += v[j] * v[j]; }
  wave_sum2(s1, s2);
  float mean, rstd;
  if constexpr (RAGGED) ln_mean_rstd_n(s1, s2, a.d, mean, rstd);
  else ln_mean_rstd<D>(s1, s2, mean, rstd);
  float d = 0.f;
#pragma unroll
  for (int j = 0; j < VPL; ++j) {   // v: the row's values, then its pre-activations, then y
    const float xh = (v[j] - mean) * rstd;
    v[j] = xh * a.gamma[pb + kStep * j] + a.beta[pb + kStep * j];
    if (a.xhat) a.xhat[(long)row * D + c0 + kStep * j] = xh;
  }
  ln_activate(a.act, v);
#pragma unroll
  for (int j = 0; j < VPL; ++j) {
    const int col = c0 + kStep * j;
    a.y[lrow * a.ld_y + (long)grp * a.y_goff + col] = v[j];
    if (a.dot_out) d += v[j] * a.dot_w[(long)grp * a.dot_gstride + col];
  }
  if (a.rstd && lane == 0) a.rstd[row] = rstd;
  if (a.dot_out) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) d += __shfl_xor(d, off);
    d += a.dot_b[(long)grp * a.dot_b_gstride];
    if (lane == 0) a.dot_out[row] = d;
  }
  return d;
}

// The LayerNorm-free ("plain") row of an MLP layer with use_layer_norm=False (mlp.py:23-31: y = act(Dense(x) + b)), in ln_row's
// lane-to-column layouts and with its gather: bias first, then the slabs in index order.  No statistics, so the row itself
// needs no exchange between lanes; the dot_out rider (the critic's Q head on its last layer) keeps ln_row's: a lane's columns in
// ascending order, then the xor butterfly.  What the backward reads: y (tanh and relu differentiate from it) and, for swish, the
// pre-activation, which goes to the layer's xhat buffer (a plain layer has no normalised row to keep there); rstd is not written.
// A launch is plain when its instances carry no gamma (LnFwdArgs); a row kernel of its own, so that ln_row's text stays what it is.
template <int VPL, bool BLOCKED>
__device__ __forceinline__ float plain_row(const LnFwdArgs& a, int row, int lane) {
  constexpr int D = 64 * VPL, kStep = kLnStep<BLOCKED>;
  const int grp = row / a.rows_per_group;
  const long lrow = row - grp * a.rows_per_group;
  const int c0 = ln_col0<VPL, BLOCKED>(lane);
  const long base = (long)grp * a.S * a.slab_stride + lrow * D + c0;
  const long pb = (long)grp * a.pstride + c0;
  float v[VPL];
  ln_gather<VPL, BLOCKED>(a, base, pb, v);
  if (a.xhat) {
#pragma unroll
    for (int j = 0; j < VPL; ++j) a.xhat[(long)row * D + c0 + kStep * j] = v[j];
  }
  ln_activate(a.act, v);
  float d = 0.f;
#pragma unroll
  for (int j = 0; j < VPL; ++j) {
    const int col = c0 + kStep * j;
    a.y[lrow * a.ld_y + (long)grp * a.y_goff + col] = v[j];
    if (a.dot_out) d += v[j] * a.dot_w[(long)grp * a.dot_gstride + col];
  }
  if (a.dot_out) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) d += __shfl_xor(d, off);
    d += a.dot_b[(long)grp * a.dot_b_gstride];
    if (lane == 0) a.dot_out[row] = d;
  }
  return d;
}

// The raw standard deviation of a std parameterisation (actor_critic_nets.py:196-211) before the clip to [std_min, std_max]
template <int MODE>
__device__ __forceinline__ float policy_std_raw(float ls) {
  return (MODE & kPolStdMask) == kPolSoftplus ? softplusf(ls) : expf(ls);
}
// kPolFixed (actor_critic_nets.py:190-192,212): the head owns no std parameter.  What the other modes call `ls` is then the
// agent's constant fixed_std vector itself, std = clip(fixed_std[j], std_min, std_max) in float32, policy_std_raw has no meaning,
// the head GEMM has one group and the second half of `pre` is neither written nor read.
template <int MODE>
__device__ __forceinline__ constexpr bool policy_fixed() { return (MODE & kPolStdMask) == kPolFixed; }
// whether the head GEMM has the log-std group behind the mean's
template <int MODE>
__device__ __forceinline__ constexpr bool policy_ls_group() { return (MODE & kPolStdMask) != kPolUniform && !policy_fixed<MODE>(); }
// std of one element from `ls` (the log-std, the softplus argument, or with kPolFixed the fixed std)
template <int MODE>
__device__ __forceinline__ float policy_std(float ls, float std_min, float std_max) {
  if (policy_fixed<MODE>()) return fminf(fmaxf(ls, std_min), std_max);
  return fminf(fmaxf(policy_std_raw<MODE>(ls), std_min), std_max);
}

// Gaussian head of rows [r0, r1) from the head GEMM's slabs (actor_critic_nets.py:179-272): one thread per (row, action).
// MODE (internal.h, kPol*): the std parameterisation, and whether the sample goes through tanh.  kPolUniform: the head GEMM has
// no log-std group -- `ls` is the shared log_stds vector (bias_ls) alone and no second slab is read.  kPolFixed: see policy_fixed.
template <bool LIVE, int MODE>
__device__ __forceinline__ void policy_dist_rows(const PolicyDistArgs& v, int r0, int r1, int tid, int nthreads) {
  const int A = v.A, B = v.B;
  const __amdgpu_buffer_rsrc_t rs = rsrc_of(v.slabs);
  for (int e = r0 * A + tid; e < r1 * A; e += nthreads) {
    const int b = e / A, j = e - b * A;
    float mean = v.bias_mean[j], ls = v.bias_ls[j];
    for (int sp = 0; sp < v.S; ++sp) {   // K-split slabs of the head GEMM: [mean | log_std][split][rows][ld]
      const long o0 = (long)sp * v.slab_stride + (long)b * v.slab_ld + j, o1 = o0 + (long)v.S * v.slab_stride;
      mean += LIVE ? ld1_sc1(rs, o0) : v.slabs[o0];
      if (policy_ls_group<MODE>()) ls += LIVE ? ld1_sc1(rs, o1) : v.slabs[o1];
    }
    float ep;
    if (v.eps) ep = v.eps[(long)b * A + j];
    else {
      ep = v.tf ? normal_from_bits(random_bits_at(v.tf_key[0], v.tf_key[1], (uint64_t)v.tf_rows * (uint64_t)A,
                                                 (uint64_t)(v.tf_row0 + b) * (uint64_t)A + (uint64_t)j))
                : hash_normal(v.seed, (uint64_t)(v.row_offset + b) * (uint64_t)A + (uint64_t)j);
      v.eps_out[(long)b * A + j] = ep;
    }
    v.pre[(long)b * A + j] = mean;
    if (!policy_fixed<MODE>()) v.pre[((long)B + b) * A + j] = ls;
    const float sd = policy_std<MODE>(ls, v.std_min, v.std_max);
    const float u = mean + sd * ep;
    v.act[(long)b * v.ld_act + j] = (MODE & kPolNoTanh) ? u : tanhf(u);
    v.std_out[(long)b * A + j] = sd;
  }
}
// logp[b] = sum_j(-eps^2/2 - log std - log(2pi)/2) - sum_j 2(log2 - u - softplus(-2u)), in j order (one thread per row); the
// second sum is the Tanh bijector's log-determinant, absent with kPolNoTanh
template <int MODE>
__device__ __forceinline__ void policy_logp_rows(const PolicyDistArgs& v, int r0, int r1, int tid, int nthreads) {
  const int A = v.A;
  for (int b = r0 + tid; b < r1; b += nthreads) {
    float lp = 0.f;
    for (int j = 0; j < A; ++j) {
      const float e = v.eps ? v.eps[(long)b * A + j] : v.eps_out[(long)b * A + j];
      const float sd = v.std_out[(long)b * A + j];
      lp += -0.5f * e * e - logf(sd) - 0.91893853320467274f;
      if (!(MODE & kPolNoTanh)) {
        const float u = v.pre[(long)b * A + j] + sd * e;
        lp -= 2.f * (0.69314718055994531f - u - softplusf(-2.f * u));
      }
    }
    v.logp[b] = lp;
  }
}
template <int MODE>
__device__ __forceinline__ void policy_tile(const PolicyDistArgs& v, int r0, int r1, int tid) {
  policy_dist_rows<true, MODE>(v, r0, r1, tid, 256);
  __syncthreads();   // (this workgroup's own global writes of pre / std / eps, read back below)
  policy_logp_rows<MODE>(v, r0, r1, tid, 256);
}
// X(MODE) for the compile-time constant equal to `mode`; `bad` for a value that is no mode.  SERL_POLICY_PARAM_CASES: the six modes
// whose std has a parameter; SERL_POLICY_MODE_SWITCH: those and the two kPolFixed ones.
#define SERL_POLICY_PARAM_CASES(X)                                             \
    case kPolExp: X(kPolExp); break;                                           \
    case kPolSoftplus: X(kPolSoftplus); break;                                 \
    case kPolUniform: X(kPolUniform); break;                                   \
    case kPolExp | kPolNoTanh: X(kPolExp | kPolNoTanh); break;                 \
    case kPolSoftplus | kPolNoTanh: X(kPolSoftplus | kPolNoTanh); break;       \
    case kPolUniform | kPolNoTanh: X(kPolUniform | kPolNoTanh); break;
#define SERL_POLICY_MODE_SWITCH(mode, X, bad)                                  \
  switch (mode) {                                                              \
    SERL_POLICY_PARAM_CASES(X)                                                 \
    case kPolFixed: X(kPolFixed); break;                                       \
    case kPolFixed | kPolNoTanh: X(kPolFixed | kPolNoTanh); break;             \
    default: bad;                                                              \
  }

// the epilogue proper; `lds` = the kernel's operand LDS (>= kEpiScratch floats + 1 int), idle after the K loop.
// (A LayerNorm + tanh reducer -- the last arriver of a 64-row tile normalising its rows -- existed in round 4: bit-identical, and
// slower in every schedule than the separate LayerNorm launch that spreads the rows over the chip; removed, numbers in
// profiles/README.md.)
template <bool ALT>
__device__ __forceinline__ void gemm_epilogue(const GemmDesc& g, const f32x16& acc, float* C, int z, int batch, int m0, int n0,
                                              float* lds, int tid) {
  store_tile_sc1(C, g.ldc, m0, n0, acc, lds, tid);
  int* flag = reinterpret_cast<int*>(lds + kEpiScratch);
  const int tiles_m = (g.M + kGBM - 1) / kGBM, tiles_n = (g.N + kGBN - 1) / kGBN;
  if (g.epi == kEpiReduce) {
    const int zg = z / g.zred;
    if (!arrive_is_last(g.ctr + ((long)zg * tiles_m + blockIdx.y) * tiles_n + blockIdx.x, g.zred, flag)) return;
    const __amdgpu_buffer_rsrc_t rs = rsrc_of(g.C + (long)zg * g.zred * g.sCz);
    float* out = g.out + (long)zg * g.out_gstride;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int m = m0 + 16 * p + (tid >> 4), n = n0 + 4 * (tid & 15);
      if (m >= g.M || n >= g.N) continue;
      f32x4 sum = {0.f, 0.f, 0.f, 0.f};
      for (int s = 0; s < g.zred; ++s) sum += ld_sc1(rs, (long)s * g.sCz + (long)m * g.ldc + n);
      float* o = out + (long)m * g.ld_out + n;
      if (n + 4 <= g.N) *reinterpret_cast<f32x4u*>(o) = sum;
      else for (int j = 0; j < g.N - n; ++j) o[j] = sum[j];
    }
  } else {   // kEpiPolicy
    if (!arrive_is_last(g.ctr + blockIdx.y, g.nbatch * g.splitk * tiles_n, flag)) return;
    const int r_end = min(m0 + kGBM, g.M);
    // ALT: the instantiations gemm_f32_multi launches for a head of another distribution than kPolExp; every other kernel holds
    // the kPolExp rows alone, the code it always held
    if (!ALT) {
      policy_tile<kPolExp>(g.pd, m0, r_end, tid);
    } else {
#define SERL_X(M) policy_tile<M>(g.pd, m0, r_end, tid)
      SERL_POLICY_MODE_SWITCH(g.pd.mode, SERL_X, break)
#undef SERL_X
    }
    if (blockIdx.y == 0 && tid == 0 && g.pd.alpha_out) g.pd.alpha_out[0] = softplusf(g.pd.lam[0]);
  }
}

// Several independent GEMMs in one launch (the chain is latency-bound: one launch per *kind* of work, not per
// instance): group i owns blockIdx.z in [zend[i-1], zend[i]); the x/y grid is the maximum over the groups.
struct GemmMulti {
  GemmDesc d[kMaxGemmGroups];
  int zend[kMaxGemmGroups];
  int n;
};

template <bool A_KFAST, bool B_KFAST, bool ALT = false>
__global__ __launch_bounds__(256) void gemm_f32_kernel(GemmMulti mm) {
  static_assert(2 * kGTile >= kEpiScratch + 4, "the epilogue's transpose scratch lives in the operand LDS");
  __shared__ __attribute__((aligned(16))) float ABf[2 * kGTile];
  float* const As = ABf;            // [m][k] (pitch 36) or [k][m] (pitch 68)
  float* const Bs = ABf + kGTile;   // [n][k]             or [k][n]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  int grp = 0;
  while (grp + 1 < mm.n && (int)blockIdx.z >= mm.zend[grp]) ++grp;
  const GemmDesc& g = mm.d[grp];
  const int z = blockIdx.z - (grp ? mm.zend[grp - 1] : 0), batch = z / g.splitk, split = z - batch * g.splitk;
  const int m0 = blockIdx.y * kGBM, n0 = blockIdx.x * kGBN;
  if (m0 >= g.M || n0 >= g.N) return;
  const int kper = ((g.K + g.splitk - 1) / g.splitk + kGBK - 1) / kGBK * kGBK;
  const int k_begin = split * kper, k_end = min(g.K, k_begin + kper);
  float* C = g.C + (long)z * g.sCz;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const int li = lane & 31, lh = lane >> 5;
  if (k_begin < k_end) {
    OperandLoader<A_KFAST> la;
    OperandLoader<B_KFAST> lb;
    la.init(g.A + (long)batch * g.sAb, g.sAm, g.sAk, m0, g.M, k_begin, tid);
    lb.init(g.B + (long)batch * g.sBb, g.sBn, g.sBk, n0, g.N, k_begin, tid);
    f32x4 ra[2], rb[2];
    la.load(ra, k_begin, k_end);
    lb.load(rb, k_begin, k_end);
    for (int k0 = k_begin; k0 < k_end; k0 += kGBK) {
      la.store(As, ra, tid);
      lb.store(Bs, rb, tid);
      __syncthreads();
      la.load(ra, k0 + kGBK, k_end);  // past k_end: all-zero vectors, nothing is dereferenced
      lb.load(rb, k0 + kGBK, k_end);
#pragma unroll
      for (int q = 0; q < kGBK / 8; ++q) {
        const f32x4 a = OperandLoader<A_KFAST>::frag(As, wm * 32 + li, lh, q);
        const f32x4 b = OperandLoader<B_KFAST>::frag(Bs, wn * 32 + li, lh, q);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[j], acc, 0, 0, 0);
      }
      __syncthreads();
    }
  }
  if (g.epi) { gemm_epilogue<ALT>(g, acc, C, z, batch, m0, n0, As, tid); return; }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
    const int n = n0 + wn * 32 + li;
    if (m < g.M && n < g.N) C[(long)m * g.ldc + n] = acc[r];
  }
}

// =============================================================================================
// The same GEMM on the bf16 matrix pipe: "bf16x3".  Every fp32 operand is split into three bf16 pieces
//     x = x0 + x1 + x2,   x0 = rn16(x), x1 = rn16(x - x0), x2 = rn16(x - x0 - x1)          (split3 below)
// (bf16 keeps fp32's exponent and 8 significant bits: three pieces cover the 24-bit significand) and the product a*b is taken
// as the six piece products with i + j <= 2
//     a0 b0 + (a0 b1 + a1 b0) + (a0 b2 + a1 b1 + a2 b0)
// on v_mfma_f32_32x32x16_bf16, accumulated in fp32; the dropped products a1 b2 + a2 b1 + a2 b2 are below 2^-23 |a b| and of
// either sign -- fp32 round-off class.  Unlike the trunk's split-fp16 scheme this needs NO operand scaling (bf16 has the
// range of fp32), so it takes activations, weights and back-propagated gradients (1e-3 .. 1e-9) alike: 6 MFMAs of 32 cycles
// per 32x32x16 block instead of 8 of 64 -- 2.7x less time on the matrix pipe, which the update chain shares with the frozen
// trunk of the next batch on the other stream.  Same descriptor, grid, K-split and epilogue as gemm_f32_kernel (drop-in);
// SERL_GEMM=f32 keeps the exact kernel as the reference arithmetic.
// LDS: per operand three planes [64 rows][32 k] bf16 (64-byte rows, 16-byte slots XOR-swizzled by (row >> 2) & 3:
// conflict-free ds_read_b128 fragments, as in the trunk kernels).  A k-contiguous operand arrives as 16-byte global
// vectors (4 k of one row -> one 8-byte store per plane); a row-contiguous operand as eight coalesced 4-byte loads per
// thread (8 consecutive k of one row, 64 consecutive rows per wave instruction -> one 16-byte store per plane).
// =============================================================================================
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// byte offset of 16-byte slot `slot` of tile row `row` in a bf16 plane with BK k's per row (BK = 32: 64-byte rows, slots
// XOR-ed with (row >> 2) & 3; BK = 16: 32-byte rows, slots XOR-ed with (row >> 3) & 1) -- conflict-free ds_read_b128
// fragments for the lane groups of MI355X_MICROARCH.md (rows {0-3, 12-15, 20-27} etc. land on 64 distinct banks)
template <int BK>
__device__ __forceinline__ int xswz(int row, int slot) {
  return BK == 32 ? row * 64 + ((slot ^ ((row >> 2) & 3)) << 4) : row * 32 + ((slot ^ ((row >> 3) & 1)) << 4);
}

// two fp32 values -> their three bf16 pieces, packed (first value in the low half).  ROUND-TO-NEAREST pieces (v_cvt_pk_bf16_f32):
// x0 = rn(x), x1 = rn(x - x0), x2 = rn(x - x0 - x1); both differences are exact in fp32 and |x1| <= 2^-8 |x|, |x2| <= 2^-16 |x|
// (x2 itself is exact unless x - x0 needs 17 bits, then it is off by < 2^-25 |x|).  Round 3 split by TRUNCATION: remainders twice
// as large and all of x's sign, so the dropped products a1 b2 + a2 b1 reached 2^-20 |a b| and biased every dot product
// towards zero; with rounded pieces they are <= 2^-23 |a b| and sign-symmetric.
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split3(float v, float w, unsigned& p0, unsigned& p1, unsigned& p2) {
  const f32x2_t x = {v, w};
  p0 = __builtin_bit_cast(unsigned, __builtin_convertvector(x, bf16x2_t));
  const f32x2_t r1 = x - (f32x2_t){__builtin_bit_cast(float, p0 << 16), __builtin_bit_cast(float, p0 & 0xffff0000u)};
  p1 = __builtin_bit_cast(unsigned, __builtin_convertvector(r1, bf16x2_t));
  const f32x2_t r2 = r1 - (f32x2_t){__builtin_bit_cast(float, p1 << 16), __builtin_bit_cast(float, p1 & 0xffff0000u)};
  p2 = __builtin_bit_cast(unsigned, __builtin_convertvector(r2, bf16x2_t));
}

// One operand tile of 64 rows x BK k's per chunk.  KFAST: 16-byte global vectors along k (BK / 16 per thread); otherwise
// BK / 4 coalesced 4-byte loads per thread: tile row tid & 63, k's (BK / 4) * (tid >> 6) + j.
template <bool KFAST, int BK, bool GATHER = false>
struct XLoader {
  static constexpr int NV = KFAST ? BK / 16 : 1;   // global vectors per thread (KFAST)
  static constexpr int NE = BK / 4;                // floats per thread per chunk
  static constexpr int kPlane = kGBM * BK * 2;     // bytes of one bf16 plane
  const float* p[NV];
  int ok[NV];   // this thread's row exists
  const float* safe = nullptr;   // the operand's first element: where loads of non-existent rows / k's are redirected
  long sK;
  int row0, kq;   // !KFAST: tile row of this thread, first k of its group
  // gather mode (GemmDesc::gtab): the operand is a virtual im2col matrix
  const int* tab = nullptr;   // KFAST: unused after init; !KFAST: row offsets, indexed by k
  int gseg = 0, gkbias = 0, gcnt = 0;
  long gpitch = 0;
  bool bias_row = false;      // !KFAST: this thread's tile row is the bias column (all ones)
  int tpre[BK / 4];           // !KFAST: row offsets of the chunk the NEXT load() call fetches (read one call ahead: the pixel loads
  int tlast = 0;              //         depend on them, and a dependent pair inside one call would make the fetch synchronous)
  // KFAST (forward): tile rows are im2col rows, k runs along a patch; !KFAST (weight gradient): tile rows are patch columns
  __device__ __forceinline__ void init_gather(const GemmDesc& g, int batch, int r0, int R, int k_begin, int tid) {
    gseg = g.gseg; gkbias = g.gkbias; gpitch = g.gpitch; sK = 1;
    safe = g.A;
    if (KFAST) {
      tab = g.gtab + (long)batch * g.M;
      const int ky = k_begin / gseg;
      gcnt = (k_begin - ky * gseg) / BK;   // chunks already consumed in the current kernel row
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int idx = tid + 256 * i, r = idx / (BK / 4);
        ok[i] = r0 + r < R;
        p[i] = g.A + (ok[i] ? tab[r0 + r] : 0) + (long)ky * gpitch + (k_begin - ky * gseg) + 4 * (idx % (BK / 4));
      }
    } else {
      tab = g.gtab + (long)batch * g.K;
      tlast = g.K - 1;
      row0 = tid & 63; kq = NE * (tid >> 6);
      const int kcol = r0 + row0;
      ok[0] = kcol < R;
      bias_row = kcol == gkbias;
      const int ky = min(kcol, gkbias - 1) / gseg;
      p[0] = g.A + (long)ky * gpitch + (min(kcol, gkbias - 1) - ky * gseg);
#pragma unroll
      for (int j = 0; j < NE; ++j) tpre[j] = tab[min(k_begin + kq + j, tlast)];   // row offsets of the FIRST chunk
    }
  }
  __device__ __forceinline__ void init(const float* X, long sR, long sK_, int r0, int R, int k_begin, int tid) {
    sK = sK_;
    safe = X;
    if (KFAST) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int idx = tid + 256 * i, r = idx / (BK / 4);
        ok[i] = r0 + r < R;
        p[i] = X + (long)(r0 + r) * sR + k_begin + 4 * (idx % (BK / 4));
      }
    } else {
      row0 = tid & 63; kq = NE * (tid >> 6);
      ok[0] = r0 + row0 < R;
      p[0] = X + (long)(k_begin + kq) * sK + r0 + row0;
    }
  }
  // the chunk starting at k0 (elements at k >= k_end are zero); advances to the next chunk
  __device__ __forceinline__ void load(float (&r)[NE], int k0, int k_end) {
    // The gather paths are BRANCH-FREE and UNTOUCHED like the plain ones below (round 4: with each load in its own exec-masked
    // region the SmallEncoder's GEMMs waited vmcnt(0) right behind every load): an element that does not exist is fetched from
    // the operand's first element and fixed at LDS-store time by clean().
    if (GATHER && KFAST) {   // gather, forward: a chunk lies inside one kernel row (gseg % BK == 0) or is the bias chunk
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int k = k0 + 4 * ((threadIdx.x + 256 * i) % (BK / 4));
        const f32x4 v = *reinterpret_cast<const f32x4u*>((ok[i] && k < gkbias) ? p[i] : safe);
        r[4 * i] = v[0]; r[4 * i + 1] = v[1]; r[4 * i + 2] = v[2]; r[4 * i + 3] = v[3];
        p[i] += BK;
      }
      if (++gcnt == gseg / BK) {   // next kernel row
        gcnt = 0;
#pragma unroll
        for (int i = 0; i < NV; ++i) p[i] += gpitch - gseg;
      }
    } else if (GATHER) {     // gather, weight gradient: k runs over the im2col rows; this chunk's row offsets were read one call ago
#pragma unroll
      for (int j = 0; j < NE; ++j) r[j] = p[0][tpre[j]];
#pragma unroll
      for (int j = 0; j < NE; ++j) tpre[j] = tab[min(k0 + BK + kq + j, tlast)];
    } else if (KFAST) {
      // BRANCH-FREE and UNTOUCHED: the load is always issued (a vector that lies outside the operand is redirected to the
      // operand's first element) and the raw registers are left alone until store() zeroes the invalid elements -- two chunks
      // later.  With the loads inside exec-masked branches (round 3), or with the zeroing selects right behind them, hipcc
      // waits vmcnt(0) in the same iteration and the "prefetch" is synchronous: ~1 us per 16-wide chunk, matrix pipe 10 % busy.
      // A partially valid vector (K % 4 != 0) reads up to 12 bytes past its row: inside the next row or the 256-byte padding
      // every arena buffer ends with.
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int krem = k_end - (k0 + 4 * ((threadIdx.x + 256 * i) % (BK / 4)));
        const f32x4 v = *reinterpret_cast<const f32x4u*>((ok[i] && krem > 0) ? p[i] : safe);
        r[4 * i] = v[0]; r[4 * i + 1] = v[1]; r[4 * i + 2] = v[2]; r[4 * i + 3] = v[3];
        p[i] += BK;
      }
    } else {
#pragma unroll
      for (int j = 0; j < NE; ++j) r[j] = *((ok[0] && k0 + kq + j < k_end) ? p[0] + (long)j * sK : safe);
      p[0] += (long)BK * sK;
    }
  }
  // zeroes the elements of chunk k0 that do not exist (rows past the operand, k >= k_end) and sets the gather operand's ones
  __device__ __forceinline__ void clean(float (&r)[NE], int k0, int k_end) const {
    if (GATHER && KFAST) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int k = k0 + 4 * ((threadIdx.x + 256 * i) % (BK / 4));
        const bool live = ok[i] && k < gkbias, one = ok[i] && k == gkbias && k < k_end;
#pragma unroll
        for (int j = 0; j < 4; ++j) r[4 * i + j] = live ? r[4 * i + j] : 0.f;
        r[4 * i] = one ? 1.0f : r[4 * i];
      }
      return;
    }
    if (GATHER) {
#pragma unroll
      for (int j = 0; j < NE; ++j) r[j] = (ok[0] && k0 + kq + j < k_end) ? (bias_row ? 1.0f : r[j]) : 0.f;
      return;
    }
    if (KFAST) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int krem = ok[i] ? k_end - (k0 + 4 * ((threadIdx.x + 256 * i) % (BK / 4))) : 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) r[4 * i + j] = krem > j ? r[4 * i + j] : 0.f;
      }
    } else {
#pragma unroll
      for (int j = 0; j < NE; ++j) r[j] = (ok[0] && k0 + kq + j < k_end) ? r[j] : 0.f;
    }
  }
  __device__ __forceinline__ void store(uint8_t* S, const float (&r)[NE], int tid) const {
    if (KFAST) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int idx = tid + 256 * i, row = idx / (BK / 4), k4 = idx % (BK / 4);
        unsigned q0[2], q1[2], q2[2];
        split3(r[4 * i], r[4 * i + 1], q0[0], q1[0], q2[0]);
        split3(r[4 * i + 2], r[4 * i + 3], q0[1], q1[1], q2[1]);
        const int off = xswz<BK>(row, k4 >> 1) + (k4 & 1) * 8;
        *reinterpret_cast<u32x2*>(S + off) = (u32x2){q0[0], q0[1]};
        *reinterpret_cast<u32x2*>(S + kPlane + off) = (u32x2){q1[0], q1[1]};
        *reinterpret_cast<u32x2*>(S + 2 * kPlane + off) = (u32x2){q2[0], q2[1]};
      }
    } else if (NE == 8) {
      unsigned q0[4], q1[4], q2[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) split3(r[2 * j], r[2 * j + 1], q0[j], q1[j], q2[j]);
      const int off = xswz<BK>(row0, kq >> 3);
      *reinterpret_cast<u32x4*>(S + off) = (u32x4){q0[0], q0[1], q0[2], q0[3]};
      *reinterpret_cast<u32x4*>(S + kPlane + off) = (u32x4){q1[0], q1[1], q1[2], q1[3]};
      *reinterpret_cast<u32x4*>(S + 2 * kPlane + off) = (u32x4){q2[0], q2[1], q2[2], q2[3]};
    } else {   // 4 k's: half a slot
      unsigned q0[2], q1[2], q2[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) split3(r[2 * j], r[2 * j + 1], q0[j], q1[j], q2[j]);
      const int off = xswz<BK>(row0, kq >> 3) + ((kq >> 2) & 1) * 8;
      *reinterpret_cast<u32x2*>(S + off) = (u32x2){q0[0], q0[1]};
      *reinterpret_cast<u32x2*>(S + kPlane + off) = (u32x2){q1[0], q1[1]};
      *reinterpret_cast<u32x2*>(S + 2 * kPlane + off) = (u32x2){q2[0], q2[1]};
    }
  }
};

// BK = 16: 12 KB of LDS per workgroup -- the update chain's GEMMs run BESIDE the frozen trunk of the next batch, whose
// conv workgroups own 131-152 KB of a CU's 160 KB: a 12 KB workgroup fits next to two row-slab (140 KB) or two LDS-DMA
// (131 KB) conv workgroups instead of waiting for one of them to retire and taking its place.
// GATHER: the SmallEncoder's implicit-GEMM operand (GemmDesc::gtab) is compiled in -- a separate instantiation, because a
// run-time "gather or not" inside the chunk loop makes every loaded value a phi and hipcc then waits right behind each load
template <bool A_KFAST, bool B_KFAST, int BK, bool GATHER = false, bool ALT = false>
__global__ __launch_bounds__(256) void gemm_bf16x3_kernel(GemmMulti mm) {
  constexpr int kPlane = kGBM * BK * 2;
  static_assert(6 * kPlane >= (kEpiScratch + 4) * 4, "the epilogue's transpose scratch lives in the operand LDS");
  __shared__ __attribute__((aligned(16))) uint8_t AB[6 * kPlane];
  uint8_t* const As = AB;
  uint8_t* const Bs = AB + 3 * kPlane;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  int grp = 0;
  while (grp + 1 < mm.n && (int)blockIdx.z >= mm.zend[grp]) ++grp;
  const GemmDesc& g = mm.d[grp];
  const int z = blockIdx.z - (grp ? mm.zend[grp - 1] : 0), batch = z / g.splitk, split = z - batch * g.splitk;
  const int m0 = blockIdx.y * kGBM, n0 = blockIdx.x * kGBN;
  if (m0 >= g.M || n0 >= g.N) return;
  const int kper = ((g.K + g.splitk - 1) / g.splitk + kGBK - 1) / kGBK * kGBK;   // (same K partition as the fp32 kernel)
  const int k_begin = split * kper, k_end = min(g.K, k_begin + kper);
  float* C = g.C + (long)z * g.sCz;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const int li = lane & 31, lh = lane >> 5;
  if (k_begin < k_end) {
    XLoader<A_KFAST, BK, GATHER> la;
    XLoader<B_KFAST, BK> lb;
    if (GATHER) la.init_gather(g, batch, m0, g.M, k_begin, tid);   // (the launcher: every group of a gather launch gathers)
    else la.init(g.A + (long)batch * g.sAb, g.sAm, g.sAk, m0, g.M, k_begin, tid);
    lb.init(g.B + (long)batch * g.sBb, g.sBn, g.sBk, n0, g.N, k_begin, tid);
    // TWO chunks in flight (register sets 0 / 1): a chunk is 4 KB per operand, its MFMAs take ~0.2 us, an L2 / Infinity-Cache
    // round trip next to the trunk pass 1-2 us -- one chunk of look-ahead left the K = 4096 bottleneck GEMM at ~1 us per chunk
    float ra[2][BK / 4], rb[2][BK / 4];
    la.load(ra[0], k_begin, k_end);
    lb.load(rb[0], k_begin, k_end);
    la.load(ra[1], k_begin + BK, k_end);  // past k_end: zeros, nothing is dereferenced
    lb.load(rb[1], k_begin + BK, k_end);
    for (int k0 = k_begin; k0 < k_end; k0 += 2 * BK) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int kk = k0 + h * BK;
        if (kk >= k_end) break;   // (uniform)
        la.clean(ra[h], kk, k_end);
        lb.clean(rb[h], kk, k_end);
        la.store(As, ra[h], tid);
        lb.store(Bs, rb[h], tid);
        __syncthreads();
        la.load(ra[h], kk + 2 * BK, k_end);
        lb.load(rb[h], kk + 2 * BK, k_end);
#pragma unroll
        for (int ks = 0; ks < BK / 16; ++ks) {
          const int ao = xswz<BK>(wm * 32 + li, 2 * ks + lh), bo = xswz<BK>(wn * 32 + li, 2 * ks + lh);
          bf16x8 a[3], b[3];
#pragma unroll
          for (int pl = 0; pl < 3; ++pl) {
            a[pl] = *reinterpret_cast<const bf16x8*>(As + pl * kPlane + ao);
            b[pl] = *reinterpret_cast<const bf16x8*>(Bs + pl * kPlane + bo);
          }
          // smallest terms first
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], acc, 0, 0, 0);
        }
        __syncthreads();
      }
    }
  }
  if (g.epi) { gemm_epilogue<ALT>(g, acc, C, z, batch, m0, n0, reinterpret_cast<float*>(AB), tid); return; }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
    const int n = n0 + wn * 32 + li;
    if (m < g.M && n < g.N) C[(long)m * g.ldc + n] = g.relu ? fmaxf(acc[r], 0.f) : acc[r];
  }
}

// arbitrary element strides: scalar loads, [k][m] LDS tiles
__global__ __launch_bounds__(256) void gemm_f32_strided_kernel(GemmDesc g) {
  constexpr int BK = 16, P = 68, LD = kGBM * BK / 256;
  __shared__ float As[BK][P];
  __shared__ float Bs[BK][P];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int z = blockIdx.z, batch = z / g.splitk, split = z - batch * g.splitk;
  const int m0 = blockIdx.y * kGBM, n0 = blockIdx.x * kGBN;
  const int kper = ((g.K + g.splitk - 1) / g.splitk + kGBK - 1) / kGBK * kGBK;
  const int k_begin = split * kper, k_end = min(g.K, k_begin + kper);
  const float* A = g.A + (long)batch * g.sAb;
  const float* B = g.B + (long)batch * g.sBb;
  float* C = g.C + (long)z * g.sCz;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const int li = lane & 31, lh = lane >> 5;
  for (int k0 = k_begin; k0 < k_end; k0 += BK) {
#pragma unroll
    for (int i = 0; i < LD; ++i) {
      const int x = tid & 63, k = (tid >> 6) + 4 * i, gk = k0 + k;
      As[k][x] = (m0 + x < g.M && gk < k_end) ? A[(long)(m0 + x) * g.sAm + (long)gk * g.sAk] : 0.f;
      Bs[k][x] = (n0 + x < g.N && gk < k_end) ? B[(long)gk * g.sBk + (long)(n0 + x) * g.sBn] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < BK / 2; ++ks)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[2 * ks + lh][wm * 32 + li], Bs[2 * ks + lh][wn * 32 + li], acc, 0, 0, 0);
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
    const int n = n0 + wn * 32 + li;
    if (m < g.M && n < g.N) C[(long)m * g.ldc + n] = acc[r];
  }
}

int gemm_f32_multi(const GemmDesc* gs, int n, hipStream_t stream) {
  SERL_REQUIRE(n >= 1 && n <= kMaxGemmGroups, "bad GEMM group count %d", n);
  GemmMulti mm{};
  mm.n = n;
  int gx = 0, gy = 0, z = 0;
  // one kernel instantiation per launch: a layout every group supports (a one-row / one-column operand fits both)
  bool a_k = true, a_m = true, b_k = true, b_n = true;
  for (int i = 0; i < n; ++i) {
    a_k = a_k && gs[i].sAk == 1; a_m = a_m && gs[i].sAm == 1;
    b_k = b_k && gs[i].sBk == 1; b_n = b_n && gs[i].sBn == 1;
  }
  const bool vec = (a_k || a_m) && (b_k || b_n);
  SERL_REQUIRE(vec || n == 1, "mixed operand layouts in a GEMM group");
  bool gather = false;   // (gather / relu descriptors exist only in the bf16x3 kernel)
  for (int i = 0; i < n; ++i) {
    gather = gather || gs[i].gtab != nullptr || gs[i].relu;
    SERL_REQUIRE(!gs[i].gtab || (gs[i].gseg > 0 && gs[i].gseg % 16 == 0 && (gs[i].sAk == 1 || gs[i].sAm == 1)), "bad gather GEMM");
    SERL_REQUIRE(!gs[i].relu || gs[i].splitk == 1, "relu epilogue with a K-split");
  }
  SERL_REQUIRE(!gather || vec, "gather GEMM needs a vector layout");
  for (int i = 0; i < n; ++i) {
    const GemmDesc& g = gs[i];
    SERL_REQUIRE(g.M > 0 && g.N > 0 && g.K > 0 && g.nbatch > 0 && g.splitk > 0, "bad GEMM shape");
    mm.d[i] = g;
    gx = std::max(gx, cdiv(g.N, kGBN));
    gy = std::max(gy, cdiv(g.M, kGBM));
    z += g.nbatch * g.splitk;
    mm.zend[i] = z;
  }
  dim3 grid(gx, gy, z);
  // SERL_GEMM=f32: the exact fp32-MFMA kernel (v_mfma_f32_32x32x2_f32) instead of bf16x3 -- A/B timing and parity runs
  static const bool exact = []() { const char* e = getenv("SERL_GEMM"); return e && e[0] == 'f'; }();
  bool any_epi = false;
  for (int i = 0; i < n; ++i) any_epi = any_epi || gs[i].epi != kEpiNone;
  SERL_REQUIRE(!any_epi || vec, "epilogue GEMMs need a vector layout");
  // a policy head of another distribution than kPolExp: its own instantiation (the head GEMM's operand layout), see gemm_epilogue
  bool alt = false;
  for (int i = 0; i < n; ++i) alt = alt || (gs[i].epi == kEpiPolicy && gs[i].pd.mode != kPolExp);
  if (alt) {
    for (int i = 0; i < n; ++i)
      SERL_REQUIRE(gs[i].epi == kEpiPolicy && gs[i].pd.mode == gs[0].pd.mode && !gs[i].gtab, "a policy-head launch mixes distributions or kinds of GEMM");
    SERL_REQUIRE(a_k && b_n, "the policy head's GEMM reads row-major activations and a row-major kernel");
    if (!exact) SERL_LAUNCH_CHAIN((gemm_bf16x3_kernel<true, false, 16, false, true>), grid, dim3(256), 0, stream, mm);
    else SERL_LAUNCH_CHAIN((gemm_f32_kernel<true, false, true>), grid, dim3(256), 0, stream, mm);
    SERL_HIP(hipGetLastError());
    return SERL_OK;
  }
  if (vec && (!exact || gather)) {   // BK = 16 (12 KB of LDS); BK = 32 (24 KB) was measured 30 us per step slower next to the trunk pass
    bool any_tab = false;
    for (int i = 0; i < n; ++i) any_tab = any_tab || gs[i].gtab != nullptr;
    for (int i = 0; i < n; ++i) SERL_REQUIRE(!any_tab || gs[i].gtab != nullptr, "a gather launch mixes gathered and plain operands");
    if (any_tab) {
      if (a_k && b_k) SERL_LAUNCH_CHAIN((gemm_bf16x3_kernel<true, true, 16, true>), grid, dim3(256), 0, stream, mm);
      else if (a_k) SERL_LAUNCH_CHAIN((gemm_bf16x3_kernel<true, false, 16, true>), grid, dim3(256), 0, stream, mm);
      else if (b_k) SERL_LAUNCH_CHAIN((gemm_bf16x3_kernel<false, true, 16, true>), grid, dim3(256), 0, stream, mm);
      else SERL_LAUNCH_CHAIN((gemm_bf16x3_kernel<false, false, 16, true>), grid, dim3(256), 0, stream, mm);
    } else if (a_k && b_k) SERL_LAUNCH_CHAIN((gemm_bf16x3_kernel<true, true, 16>), grid, dim3(256), 0, stream, mm);
    else if (a_k) SERL_LAUNCH_CHAIN((gemm_bf16x3_kernel<true, false, 16>), grid, dim3(256), 0, stream, mm);
    else if (b_k) SERL_LAUNCH_CHAIN((gemm_bf16x3_kernel<false, true, 16>), grid, dim3(256), 0, stream, mm);
    else SERL_LAUNCH_CHAIN((gemm_bf16x3_kernel<false, false, 16>), grid, dim3(256), 0, stream, mm);
  } else if (vec) {
    if (a_k && b_k) SERL_LAUNCH_CHAIN((gemm_f32_kernel<true, true>), grid, dim3(256), 0, stream, mm);
    else if (a_k) SERL_LAUNCH_CHAIN((gemm_f32_kernel<true, false>), grid, dim3(256), 0, stream, mm);
    else if (b_k) SERL_LAUNCH_CHAIN((gemm_f32_kernel<false, true>), grid, dim3(256), 0, stream, mm);
    else SERL_LAUNCH_CHAIN((gemm_f32_kernel<false, false>), grid, dim3(256), 0, stream, mm);
  } else {
    for (int i = 0; i < n; ++i) {
      const GemmDesc& g = gs[i];
      SERL_LAUNCH_CHAIN(gemm_f32_strided_kernel, dim3(cdiv(g.N, kGBN), cdiv(g.M, kGBM), g.nbatch * g.splitk), dim3(256), 0,
                         stream, g);
    }
  }
  SERL_HIP(hipGetLastError());
  return SERL_OK;
}

int gemm_f32(const GemmDesc& g, hipStream_t stream) { return gemm_f32_multi(&g, 1, stream); }

// out[g][row][col] (+)= bias[g][col] + sum_s slab[g*S + s][row][col]
__global__ void reduce_slabs_kernel(const float* slabs, int S, long slab_stride, int rows, int N,
                                    const float* bias, long bias_gstride, float* out, long ld_out,
                                    long out_gstride, int accumulate, float scale) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int grp = blockIdx.y;
  if (e >= (long)rows * N) return;
  const int row = (int)(e / N), col = (int)(e - (long)row * N);
  float v = 0.f;
  for (int s = 0; s < S; ++s) v += slabs[((long)grp * S + s) * slab_stride + e];
  v *= scale;
  if (bias) v += bias[(long)grp * bias_gstride + col];
  float* o = out + (long)grp * out_gstride + (long)row * ld_out + col;
  *o = accumulate ? *o + v : v;
}

int reduce_slabs(const float* slabs, int S, long slab_stride, int groups, int rows, int N, const float* bias,
                 long bias_gstride, float* out, long ld_out, long out_gstride, bool accumulate,
                 hipStream_t stream, float scale) {
  dim3 grid(cdiv((long)rows * N, 256), groups);
  SERL_LAUNCH_CHAIN(reduce_slabs_kernel, grid, dim3(256), 0, stream, slabs, S, slab_stride, rows, N, bias,
                     bias_gstride, out, ld_out, out_gstride, accumulate ? 1 : 0, scale);
  SERL_HIP(hipGetLastError());
  return SERL_OK;
}

// =============================================================================================
// LayerNorm(eps 1e-6, fast variance) + activation, one wave per row (ln_row), four rows per workgroup.
// =============================================================================================
template <int VPL, bool BLOCKED>
__global__ __launch_bounds__(256) void ln_fwd_kernel(Multi<LnFwdArgs> mv) {
  const LnFwdArgs& a = mv.v[blockIdx.y];  // blockIdx.y = independent instance (variant)
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.rows) return;
  ln_row<VPL, BLOCKED>(a, row, lane);
}
// ... of a launch in which an instance has Dropout (mlp.py:27-28): the same rows with the mask in front of the statistics
template <int VPL, bool BLOCKED>
__global__ __launch_bounds__(256) void ln_fwd_drop_kernel(Multi<LnFwdArgs> mv) {
  const LnFwdArgs& a = mv.v[blockIdx.y];
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.rows) return;
  ln_row<VPL, BLOCKED, true>(a, row, lane);
}
// ... of a launch whose instances are zero-padded rows of a true width off the 64 grid (LnFwdArgs::d)
template <int VPL, bool BLOCKED>
__global__ __launch_bounds__(256) void ln_fwd_ragged_kernel(Multi<LnFwdArgs> mv) {
  const LnFwdArgs& a = mv.v[blockIdx.y];
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.rows) return;
  ln_row<VPL, BLOCKED, false, true>(a, row, lane);
}
// ... of a launch whose instances are LayerNorm-free layers (mlp.py:29-30, use_layer_norm=False): plain_row in the same grid
template <int VPL, bool BLOCKED>
__global__ __launch_bounds__(256) void plain_fwd_kernel(Multi<LnFwdArgs> mv) {
  const LnFwdArgs& a = mv.v[blockIdx.y];
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.rows) return;
  plain_row<VPL, BLOCKED>(a, row, lane);
}

// The reward classifier's head closed for labelling (vice.py:546,594: rewards = (sigmoid(classifier(next_obs)) >= 0.5) * 1.0): the
// LayerNorm -> ReLU -> Dense(1) row of ln_row at width 256 (one row per wave; the logit goes to a.dot_out as in the train=False
// forward), then p = 1 / (1 + expf(-logit)) in fp32 (as jax.nn.sigmoid: a logit just below zero may round to 0.5) and
// label = p >= 0.5f.  The mean label is taken inside the launch by the workgroup that arrives last (arrive_is_last: write-through
// label stores, every wave drains, one ticket; the labels are read back past the L1): 256 strided partial sums in row order, then
// a halving tree -- a fixed order, whichever workgroup is last.  Rows >= a.rows of the last workgroup compute nothing but arrive.
__global__ __launch_bounds__(256) void label_rows_kernel(LnFwdArgs a, float* label, float* mean, int* ctr) {
  __shared__ float red[256 + 1];   // partial sums and, behind them, the "I am last" flag (one LDS object)
  const int tid = threadIdx.x, row = blockIdx.x * 4 + (tid >> 6), lane = tid & 63;
  const __amdgpu_buffer_rsrc_t lab = rsrc_of(label);
  if (row < a.rows) {
    const float logit = ln_row<4, true>(a, row, lane);
    const float p = 1.f / (1.f + expf(-logit));
    if (lane == 0) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, p >= 0.5f ? 1.f : 0.f), lab, row * 4, 0, kSc1);
  }
  if (!arrive_is_last(ctr, (int)gridDim.x, reinterpret_cast<int*>(&red[256]))) return;
  float s = 0.f;
  for (int r = tid; r < a.rows; r += 256) s += ld1_sc1(lab, r);
  red[tid] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) mean[0] = red[0] / (float)a.rows;
}

int label_rows(const LnFwdArgs& a, float* label, float* mean, int* ctr, hipStream_t stream) {
  SERL_REQUIRE(a.rows >= 1 && a.rows == a.rows_per_group && a.act == kActRelu && a.dot_out && label && mean && ctr, "bad label launch");
  SERL_LAUNCH_CHAIN(label_rows_kernel, dim3(cdiv(a.rows, 4)), dim3(256), 0, stream, a, label, mean, ctr);
  SERL_HIP(hipGetLastError());
  return SERL_OK;
}

// The widths the LayerNorm rows serve: one wave per row, D / 64 columns per lane, at most 16.  The launch of a width: K64 at 64
// and K256 at 256 (the encoder's proprio and bottleneck LayerNorms, and the MLPs at the default width), the strided K<D / 64, false>
// at every other.
#define SERL_LN_WIDTH_OK(D) ((D) >= 64 && (D) <= 1024 && (D) % 64 == 0)
// a launch's Dropout description: none, or a keep probability in (0, 1] with the mask tensor / the window of `rows` rows inside
// the array the key draws
static bool ln_drop_ok(const LnDrop& d, long rows) {
  if (d.mode == kLnDropNone) return true;
  if (!(d.keep > 0.f && d.keep <= 1.f)) return false;
  if (d.mode == kLnDropMask) return d.mask != nullptr;
  if (d.mode == kLnDropKey) return d.row0 >= 0 && d.row0 + rows <= d.total_rows;
  return d.mode == kLnDropHash && d.row0 >= 0;
}
#define SERL_LN_CASE(V, K, ...) case V: SERL_LAUNCH_CHAIN(K, __VA_ARGS__); break;
#define SERL_LN_STRIDED(V, K, ...) SERL_LN_CASE(V, (K<V, false>), __VA_ARGS__)
#define SERL_LN_LAUNCH(D, K64, K256, K, ...)                                                                              \
  switch ((D) / 64) {                                                                                                     \
    SERL_LN_CASE(1, K64, __VA_ARGS__) SERL_LN_CASE(4, K256, __VA_ARGS__)                                                  \
    SERL_LN_STRIDED(2, K, __VA_ARGS__) SERL_LN_STRIDED(3, K, __VA_ARGS__) SERL_LN_STRIDED(5, K, __VA_ARGS__)              \
    SERL_LN_STRIDED(6, K, __VA_ARGS__) SERL_LN_STRIDED(7, K, __VA_ARGS__) SERL_LN_STRIDED(8, K, __VA_ARGS__)              \
    SERL_LN_STRIDED(9, K, __VA_ARGS__) SERL_LN_STRIDED(10, K, __VA_ARGS__) SERL_LN_STRIDED(11, K, __VA_ARGS__)            \
    SERL_LN_STRIDED(12, K, __VA_ARGS__) SERL_LN_STRIDED(13, K, __VA_ARGS__) SERL_LN_STRIDED(14, K, __VA_ARGS__)           \
    SERL_LN_STRIDED(15, K, __VA_ARGS__) SERL_LN_STRIDED(16, K, __VA_ARGS__)                                               \
    default: serl::set_error("LayerNorm width %d has no kernel", (int)(D)); return SERL_ERR_INVALID;                      \
  }

int ln_fwd_multi(const LnFwdArgs* as, int n, int D, hipStream_t stream) {
  SERL_REQUIRE(SERL_LN_WIDTH_OK(D), "LayerNorm width %d unsupported (a multiple of 64 in [64, 1024])", D);
  SERL_REQUIRE(n >= 1 && n <= kMaxMulti, "bad instance count %d", n);
  Multi<LnFwdArgs> mv{};
  int rows = 0;
  bool drop = false;
  for (int i = 0; i < n; ++i) {
    // (the instances of a launch are evaluations of ONE layer: all of them are ragged, at one true width, or none is)
    SERL_REQUIRE(as[i].d == as[0].d && as[i].d >= 0 && as[i].d < D, "LayerNorm row: instance %d has the true width %d, instance 0 %d, in rows of %d",
                 i, as[i].d, as[0].d, D);
    SERL_REQUIRE(as[i].act >= 0 && as[i].act < kActCount, "LayerNorm row: activation code %d is not tanh (0), relu (1) or swish (2)", as[i].act);
    SERL_REQUIRE(ln_drop_ok(as[i].drop, as[i].rows_per_group), "LayerNorm row: bad Dropout description (mode %d, keep %g)", as[i].drop.mode, as[i].drop.keep);
    mv.v[i] = as[i];
    rows = std::max(rows, as[i].rows);
    drop = drop || as[i].drop.mode != kLnDropNone;
    // (the instances of a launch are evaluations of ONE layer: all of them have a LayerNorm, or none has)
    SERL_REQUIRE((as[i].gamma == nullptr) == (as[0].gamma == nullptr) && (as[i].gamma == nullptr) == (as[i].beta == nullptr),
                 "LayerNorm row: instance %d %s a LayerNorm and instance 0 %s; plain and LayerNorm rows do not share a launch", i,
                 as[i].gamma ? "has" : "lacks", as[0].gamma ? "has" : "lacks");
  }
  dim3 grid(cdiv(rows, 4), n);
  if (!as[0].gamma) {
    SERL_REQUIRE(!drop, "plain row (no LayerNorm) with Dropout: not served");
    SERL_LN_LAUNCH(D, (plain_fwd_kernel<1, false>), (plain_fwd_kernel<4, true>), plain_fwd_kernel, grid, dim3(256), 0, stream, mv)
  } else if (as[0].d) {
    SERL_REQUIRE(!drop, "ragged LayerNorm row (true width %d in %d) with Dropout: not served", as[0].d, D);
    SERL_LN_LAUNCH(D, (ln_fwd_ragged_kernel<1, false>), (ln_fwd_ragged_kernel<4, true>), ln_fwd_ragged_kernel, grid, dim3(256), 0, stream, mv)
  } else if (drop) SERL_LN_LAUNCH(D, (ln_fwd_drop_kernel<1, false>), (ln_fwd_drop_kernel<4, true>), ln_fwd_drop_kernel, grid, dim3(256), 0, stream, mv)
  else SERL_LN_LAUNCH(D, (ln_fwd_kernel<1, false>), (ln_fwd_kernel<4, true>), ln_fwd_kernel, grid, dim3(256), 0, stream, mv)
  SERL_HIP(hipGetLastError());
  return SERL_OK;
}

// REDQ target of sample b (sac.py:150-176): y = r + discount * mask * min over the selected (or all) target members
// [- alpha * log pi(a'|s') with backup_entropy, outside the discount as the reference has it]
__device__ __forceinline__ float redq_target(const LossArgs& L, int b) {
  float mq;
  if (L.sel.n > 0) {
    mq = L.qt[(long)L.sel.idx[0] * L.B + b];
    for (int k = 1; k < L.sel.n; ++k) mq = fminf(mq, L.qt[(long)L.sel.idx[k] * L.B + b]);
  } else {
    mq = L.qt[b];
    for (int e = 1; e < L.E; ++e) mq = fminf(mq, L.qt[(long)e * L.B + b]);
  }
  float y = L.reward[b] + L.discount * L.mask[b] * mq;
  if (L.logp_next) y -= L.alpha[0] * L.logp_next[b];
  return y;
}

// critic loss by ONE workgroup of 256 threads (deterministic reductions); the body of critic_loss_kernel
__device__ void critic_loss_body(const LossArgs& L, float (*red)[256]) {
  float s_d2 = 0.f, s_q = 0.f, s_y = 0.f, s_dq = 0.f;
  float s_e[16];  // per-member sums of dQ (per_member: E <= 16)
#pragma unroll
  for (int e = 0; e < 16; ++e) s_e[e] = 0.f;
  for (int b = threadIdx.x; b < L.B; b += 256) {
    const float y = redq_target(L, b);
    L.y_out[b] = y;
    s_y += y;
    for (int e = 0; e < L.E; ++e) {
      const float qv = L.q[(long)e * L.B + b];
      const float d = qv - y;
      const float g = 2.f * d * L.inv_norm;
      L.dq[(long)e * L.B + b] = g;
      s_d2 += d * d;
      s_q += qv;
      s_dq += g;
      if (L.per_member) {
#pragma unroll
        for (int k = 0; k < 16; ++k)
          if (k == e) s_e[k] += g;
      }
    }
  }
  red[0][threadIdx.x] = s_d2; red[1][threadIdx.x] = s_q; red[2][threadIdx.x] = s_y; red[3][threadIdx.x] = s_dq;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o)
      for (int k = 0; k < 4; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    L.scalars[0] = red[0][0]; L.scalars[1] = red[1][0]; L.scalars[2] = red[2][0];
    if (!L.per_member) *L.dbias = red[3][0];
  }
  if (L.per_member) {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      if (k < L.E) {  // (uniform)
        __syncthreads();
        red[0][threadIdx.x] = s_e[k];
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
          if ((int)threadIdx.x < o) red[0][threadIdx.x] += red[0][threadIdx.x + o];
          __syncthreads();
        }
        if (threadIdx.x == 0) L.dbias[k] = red[0][0];
      }
    }
  }
}

// backward of ONE row of y = act(gamma*xhat + beta), xhat = (x-mean)*rstd, by one wave, in the lane-to-column layout of ln_row:
//   dg = dy*act'(pre) (ln_act_grad; tanh: dy*(1-y^2));  dxhat = dg*gamma;  dx = rstd*(dxhat - mean(dxhat) - xhat*mean(dxhat*xhat))
// a lane sums its columns in ascending order, then the xor butterfly.  L: the launch's critic loss, read by a dq_inline row alone.
// RAGGED: a zero-padded row of true width a.d < D (heads.h).  dy is 0 in the pads (the rows of the consumer's kernel are), so dg,
// dxhat and both sums are what the d live columns give; the means divide by a.d, and dx is 0 in the pads.
template <int VPL, bool BLOCKED, bool DROP = false, bool RAGGED = false>
__device__ __forceinline__ void ln_bwd_row(const LnBwdArgs& a, const LossArgs& L, int row, int lane) {
  const int grp = row / a.rows_per_group;
  constexpr int D = VPL * 64;
  float dg[VPL], dxh[VPL], xh[VPL], y[VPL], gam[VPL];
  float s1 = 0.f, s2 = 0.f;
  const long lr = row - grp * a.rows_per_group;
  const int c0 = ln_col0<VPL, BLOCKED>(lane);
  float dqr = 0.f;
  if (a.dq_w) dqr = a.dq_inline ? 2.f * (L.q[row] - redq_target(L, (int)lr)) * L.inv_norm : (a.dq ? a.dq[row] : a.dq_const);
#pragma unroll
  for (int j = 0; j < VPL; ++j) {
    const int col = c0 + kLnStep<BLOCKED> * j;
    y[j] = a.y[lr * a.ld_y + (long)grp * a.y_goff + col];
    dg[j] = a.dq_w ? dqr * a.dq_w[(long)grp * a.dq_w_gstride + col] : a.dy[lr * a.ld_dy + (long)grp * a.dy_goff + col];
    xh[j] = a.xhat[(long)row * D + col];
    gam[j] = a.gamma[(long)grp * a.pstride + col];
  }
  ln_act_grad<VPL, BLOCKED ? 1 : 64>(a.act, dg, y, xh, gam, a.beta, (long)grp * a.pstride + c0);
#pragma unroll
  for (int j = 0; j < VPL; ++j) {
    dxh[j] = dg[j] * gam[j];
    s1 += dxh[j];
    s2 += dxh[j] * xh[j];
  }
  wave_sum2(s1, s2);
  float m1, m2;
  if constexpr (RAGGED) { const float inv = 1.0f / (float)a.d; m1 = s1 * inv; m2 = s2 * inv; }
  else { m1 = s1 * (1.0f / D); m2 = s2 * (1.0f / D); }
  const float rstd = a.rstd[row];
  if constexpr (RAGGED) {
    static_assert(!DROP, "a ragged row carries no Dropout");
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
      const int col = c0 + kLnStep<BLOCKED> * j;
      a.dx[(long)row * D + col] = col < a.d ? rstd * (dxh[j] - m1 - xh[j] * m2) : 0.f;
      a.dg[(long)row * D + col] = dg[j];
    }
  } else if constexpr (!DROP) {
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
      const int col = c0 + kLnStep<BLOCKED> * j;
      a.dx[(long)row * D + col] = rstd * (dxh[j] - m1 - xh[j] * m2);
      a.dg[(long)row * D + col] = dg[j];
    }
  } else {   // dx wrt the LayerNorm's input, then -- the forward's keep decision stated again -- wrt the Dense output in front of the Dropout
#pragma unroll
    for (int j = 0; j < VPL; ++j) dxh[j] = rstd * (dxh[j] - m1 - xh[j] * m2);
    if (a.drop.mode != kLnDropNone) ln_dropout<VPL, BLOCKED>(a.drop, lr, c0, dxh);
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
      const int col = c0 + kLnStep<BLOCKED> * j;
      a.dx[(long)row * D + col] = dxh[j];
      a.dg[(long)row * D + col] = dg[j];
    }
  }
}

// backward of ONE plain row y = act(pre) (plain_row) by one wave, in the same layout: dpre = dy * act'.  tanh: 1 - y^2; ReLU: y > 0
// (0 at 0, as jax.nn.relu's); swish: sigma(pre) + y (1 - sigma(pre)) with the pre-activation the forward row kept in xhat (read on
// this path alone).  dy in ln_bwd_row's three forms: a tensor, the rank-1 dq (x) w, and dq derived inline from the launch's loss.
// No row statistics, no exchange between lanes.  dg and dpre coincide: the row writes dx alone, and the bias's column sum and the
// weight and input gradients all read it (layer_colsum, dense_layer.h); a.dg, a.rstd, a.gamma and a.beta are not touched.
template <int VPL, bool BLOCKED>
__device__ __forceinline__ void plain_bwd_row(const LnBwdArgs& a, const LossArgs& L, int row, int lane) {
  const int grp = row / a.rows_per_group;
  constexpr int D = VPL * 64, kStep = kLnStep<BLOCKED>;
  float dg[VPL], y[VPL];
  const long lr = row - grp * a.rows_per_group;
  const int c0 = ln_col0<VPL, BLOCKED>(lane);
  float dqr = 0.f;
  if (a.dq_w) dqr = a.dq_inline ? 2.f * (L.q[row] - redq_target(L, (int)lr)) * L.inv_norm : (a.dq ? a.dq[row] : a.dq_const);
#pragma unroll
  for (int j = 0; j < VPL; ++j) {
    const int col = c0 + kStep * j;
    y[j] = a.y[lr * a.ld_y + (long)grp * a.y_goff + col];
    dg[j] = a.dq_w ? dqr * a.dq_w[(long)grp * a.dq_w_gstride + col] : a.dy[lr * a.ld_dy + (long)grp * a.dy_goff + col];
  }
  if (a.act == kActTanh) {
#pragma unroll
    for (int j = 0; j < VPL; ++j) dg[j] *= 1.f - y[j] * y[j];
  } else if (a.act == kActRelu) {
#pragma unroll
    for (int j = 0; j < VPL; ++j) dg[j] = y[j] > 0.f ? dg[j] : 0.f;
  } else {
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
      const float sg = sigmoid_stable(a.xhat[(long)row * D + c0 + kStep * j]);
      dg[j] *= sg + y[j] * (1.f - sg);
    }
  }
#pragma unroll
  for (int j = 0; j < VPL; ++j) a.dx[(long)row * D + c0 + kStep * j] = dg[j];
}

// A LayerNorm-backward launch: blockIdx.y = instance, one wave per row, four rows per workgroup; the LAST workgroup of instance 0
// is the critic-loss rider when loss.on.  VPL > 0: every instance has the width 64 * VPL (the MLP layers at a hidden width other
// than 256).  VPL == 0: instances of width 256 or 64, each its own (the encoder heads: the cameras' bottleneck and the proprio
// branch in one launch; and the MLP layers at the default width).
constexpr int kLnMixed = 0;
template <int VPL, bool BLOCKED>
__global__ __launch_bounds__(256) void ln_bwd_kernel(Multi<LnBwdArgs> mv, LossArgs loss) {
  __shared__ float red[4][256];
  if (loss.on && blockIdx.y == 0 && blockIdx.x == gridDim.x - 1) { critic_loss_body(loss, red); return; }
  const LnBwdArgs& a = mv.v[blockIdx.y];
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.rows) return;
  if constexpr (VPL != kLnMixed) ln_bwd_row<VPL, BLOCKED>(a, loss, row, lane);
  else if (a.D == 256) ln_bwd_row<4, true>(a, loss, row, lane);
  else ln_bwd_row<1, false>(a, loss, row, lane);
}

// ... of a launch in which an instance has Dropout: the rows mask dx as the forward masked the Dense output
template <int VPL, bool BLOCKED>
__global__ __launch_bounds__(256) void ln_bwd_drop_kernel(Multi<LnBwdArgs> mv, LossArgs loss) {
  __shared__ float red[4][256];
  if (loss.on && blockIdx.y == 0 && blockIdx.x == gridDim.x - 1) { critic_loss_body(loss, red); return; }
  const LnBwdArgs& a = mv.v[blockIdx.y];
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.rows) return;
  if constexpr (VPL != kLnMixed) ln_bwd_row<VPL, BLOCKED, true>(a, loss, row, lane);
  else if (a.D == 256) ln_bwd_row<4, true, true>(a, loss, row, lane);
  else ln_bwd_row<1, false, true>(a, loss, row, lane);
}

// ... of a launch whose instances are zero-padded rows of one true width off the 64 grid (LnBwdArgs::d), all of them stored
// 64 * VPL wide (an MLP layer is alone in its launch: no mixed widths); the critic-loss rider in the same place
template <int VPL, bool BLOCKED>
__global__ __launch_bounds__(256) void ln_bwd_ragged_kernel(Multi<LnBwdArgs> mv, LossArgs loss) {
  __shared__ float red[4][256];
  if (loss.on && blockIdx.y == 0 && blockIdx.x == gridDim.x - 1) { critic_loss_body(loss, red); return; }
  const LnBwdArgs& a = mv.v[blockIdx.y];
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.rows) return;
  ln_bwd_row<VPL, BLOCKED, false, true>(a, loss, row, lane);
}

// ... of a launch whose instances are LayerNorm-free layers, all of the width 64 * VPL (an MLP layer is alone in its launch):
// plain_bwd_row in the same grid, the critic-loss rider in the same place
template <int VPL, bool BLOCKED>
__global__ __launch_bounds__(256) void plain_bwd_kernel(Multi<LnBwdArgs> mv, LossArgs loss) {
  __shared__ float red[4][256];
  if (loss.on && blockIdx.y == 0 && blockIdx.x == gridDim.x - 1) { critic_loss_body(loss, red); return; }
  const LnBwdArgs& a = mv.v[blockIdx.y];
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.rows) return;
  plain_bwd_row<VPL, BLOCKED>(a, loss, row, lane);
}

// One instance of a default width without a rider (most LayerNorm backward launches of the default agent, BC, the classifier):
// the same row behind a launch that carries one LnBwdArgs (ln_bwd_kernel's arguments are four of them and the loss).  Measured:
// with ln_bwd_kernel in its place the update step is 0.36 % slower (profiles/README.md).
template <int VPL, bool BLOCKED>
__global__ __launch_bounds__(256) void ln_bwd_one_kernel(LnBwdArgs a) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.rows) return;
  ln_bwd_row<VPL, BLOCKED>(a, LossArgs{}, row, lane);   // (no dq_inline without a loss: ln_bwd_multi checks)
}

int ln_bwd_multi(const LnBwdArgs* as, int n, const LossArgs& loss, hipStream_t stream) {
  SERL_REQUIRE(n >= 1 && n <= kMaxMulti, "bad instance count %d", n);
  Multi<LnBwdArgs> mv{};
  int rows = 0;
  bool drop = false;
  const auto mixes = [](int D) { return D == 64 || D == 256; };
  for (int i = 0; i < n; ++i) {
    SERL_REQUIRE(SERL_LN_WIDTH_OK(as[i].D), "LayerNorm width %d unsupported (a multiple of 64 in [64, 1024])", as[i].D);
    // (a ragged launch is one MLP layer: one storage width, one true width, no Dropout)
    SERL_REQUIRE(as[i].d >= 0 && as[i].d < as[i].D && as[i].d == as[0].d && (!as[i].d || (as[i].D == as[0].D && as[i].drop.mode == kLnDropNone)),
                 "LayerNorm backward: instance %d has the true width %d in rows of %d, instance 0 %d in rows of %d; or a ragged row with Dropout",
                 i, as[i].d, as[i].D, as[0].d, as[0].D);
    SERL_REQUIRE(!as[i].dq_inline || (loss.on && as[i].dq_w && as[i].rows == loss.E * loss.B && as[i].rows_per_group == loss.B),
                 "inline dQ needs the loss arguments of the launch");
    // (the swish backward recomputes its pre-activation: it reads beta where the forward did)
    // (... and a plain row reads the pre-activation its forward kept in xhat)
    SERL_REQUIRE(as[i].act >= 0 && as[i].act < kActCount && (as[i].act != kActSwish || (as[i].gamma ? as[i].beta : as[i].xhat)),
                 "LayerNorm backward: activation code %d is not tanh (0), relu (1) or swish (2), or swish without beta", as[i].act);
    // (the instances of a plain launch are evaluations of one MLP layer: no LayerNorm in any, one width, no Dropout)
    SERL_REQUIRE((as[i].gamma == nullptr) == (as[0].gamma == nullptr) && (as[i].gamma || (as[i].D == as[0].D && as[i].drop.mode == kLnDropNone)),
                 "LayerNorm backward: plain and LayerNorm rows in one launch, or plain rows of widths %d and %d, or with Dropout", as[0].D, as[i].D);
    SERL_REQUIRE(ln_drop_ok(as[i].drop, as[i].rows_per_group), "LayerNorm backward: bad Dropout description (mode %d, keep %g)", as[i].drop.mode, as[i].drop.keep);
    mv.v[i] = as[i];
    rows = std::max(rows, as[i].rows);
    drop = drop || as[i].drop.mode != kLnDropNone;
    // (64 and 256 may share a launch -- the encoder heads; any other width comes from one MLP layer and is alone)
    SERL_REQUIRE(as[i].D == as[0].D || (mixes(as[i].D) && mixes(as[0].D)),
                 "LayerNorm widths %d and %d in one launch: widths other than 64 and 256 do not mix", as[0].D, as[i].D);
  }
  const dim3 grid(cdiv(rows, 4) + (loss.on ? 1 : 0), n);
  if (!as[0].gamma) SERL_LN_LAUNCH(as[0].D, (plain_bwd_kernel<1, false>), (plain_bwd_kernel<4, true>), plain_bwd_kernel, grid, dim3(256), 0, stream, mv, loss)
  else if (as[0].d) SERL_LN_LAUNCH(as[0].D, (ln_bwd_ragged_kernel<1, false>), (ln_bwd_ragged_kernel<4, true>), ln_bwd_ragged_kernel, grid, dim3(256), 0, stream, mv, loss)
  else if (drop) SERL_LN_LAUNCH(as[0].D, (ln_bwd_drop_kernel<kLnMixed, false>), (ln_bwd_drop_kernel<kLnMixed, false>), ln_bwd_drop_kernel, grid, dim3(256), 0, stream, mv, loss)
  else if (n == 1 && !loss.on && as[0].D == 256) SERL_LAUNCH_CHAIN((ln_bwd_one_kernel<4, true>), grid, dim3(256), 0, stream, as[0]);
  else if (n == 1 && !loss.on && as[0].D == 64) SERL_LAUNCH_CHAIN((ln_bwd_one_kernel<1, false>), grid, dim3(256), 0, stream, as[0]);
  else SERL_LN_LAUNCH(as[0].D, (ln_bwd_kernel<kLnMixed, false>), (ln_bwd_kernel<kLnMixed, false>), ln_bwd_kernel, grid, dim3(256), 0, stream, mv, loss)
  SERL_HIP(hipGetLastError());
  return SERL_OK;
}

// out[g][col] (+)= sum_{r in group g} X[r][col] * (Y ? Y[r][col] : 1)     (bias / LN-param grads)
__global__ __launch_bounds__(256) void colsum_kernel(const float* X, const float* Y, int rows_per_group,
                                                    int D, float* out, long out_gstride, int accumulate) {
  __shared__ float red[4][64];
  const int grp = blockIdx.y, col = blockIdx.x * 64 + (threadIdx.x & 63), part = threadIdx.x >> 6;
  float s = 0.f;
  if (col < D) {
    const long base = (long)grp * rows_per_group;
    for (int r = part; r < rows_per_group; r += 4) {
      const float x = X[(base + r) * D + col];
      s += Y ? x * Y[(base + r) * D + col] : x;
    }
  }
  red[part][threadIdx.x & 63] = s;
  __syncthreads();
  if (part == 0 && col < D) {
    const float t = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    float* o = out + (long)grp * out_gstride + col;
    *o = accumulate ? *o + t : t;
  }
}

int colsum(const float* X, const float* Y, int groups, int rows_per_group, int D, float* out,
           long out_gstride, bool accumulate, hipStream_t stream) {
  SERL_LAUNCH_CHAIN(colsum_kernel, dim3(cdiv(D, 64), groups), dim3(256), 0, stream, X, Y, rows_per_group, D,
                     out, out_gstride, accumulate ? 1 : 0);
  SERL_HIP(hipGetLastError());
  return SERL_OK;
}

// fused parameter gradients of one Dense->LN->tanh layer (one pass over dg, xhat, dpre):
//   dgamma[g][j] = sum_r dg*xhat,  dbeta[g][j] = sum_r dg,  dbias[g][j] = sum_r dpre
struct ColsumMulti { Colsum3Args v[kMaxColsum]; };
__global__ __launch_bounds__(512) void colsum3_kernel(ColsumMulti mv) {
  const Colsum3Args& a = mv.v[blockIdx.z];  // blockIdx.z = layer
  __shared__ float red[3][8][64];
  const int grp = blockIdx.y, col = blockIdx.x * 64 + (threadIdx.x & 63), part = threadIdx.x >> 6;
  if (grp >= a.groups || (int)blockIdx.x * 64 >= a.D) return;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  if (a.mode == 2) {   // a vector's sum (loss scalars), in the order policy_dist_fwd_kernel sums log-probs: 256 strided partial
    float* r1 = &red[0][0][0];   // sums, then a halving tree (fused and un-fused chains agree to the bit)
    if (threadIdx.x < 256) {
      for (int r = threadIdx.x; r < a.rows_per_group; r += 256) s1 += a.dg[r];
      r1[threadIdx.x] = s1;
    }
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) r1[threadIdx.x] += r1[threadIdx.x + o];
      __syncthreads();
    }
    if (threadIdx.x == 0) a.o_beta[0] = r1[0];
    return;
  }
  if (col < a.D) {
    const long base = (long)grp * a.rows_per_group;
    if (a.mode == 1) {   // (four row phases combined as colsum_kernel combines them)
      if (part < 4)
        for (int r = part; r < a.rows_per_group; r += 4) s1 += a.dg[(base + r) * a.D + col];
    } else {
      for (int r = part; r < a.rows_per_group; r += 8) {
        const long e = (base + r) * a.D + col;
        const float g = a.dg[e];
        s0 += g * a.xhat[e];
        s1 += g;
        s2 += a.dpre[e];
      }
    }
  }
  red[0][part][threadIdx.x & 63] = s0;
  red[1][part][threadIdx.x & 63] = s1;
  red[2][part][threadIdx.x & 63] = s2;
  __syncthreads();
  if (a.mode == 1) {
    if (part == 1 && col < a.D) {
      const int c = threadIdx.x & 63;
      a.o_beta[(long)grp * a.gstride + col] = (red[1][0][c] + red[1][1][c]) + (red[1][2][c] + red[1][3][c]);
    }
    return;
  }
  if (part < 3 && col < a.D) {
    const int c = threadIdx.x & 63;
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) t += red[part][k][c];
    float* o = (part == 0 ? a.o_gamma : (part == 1 ? a.o_beta : a.o_bias)) + (long)grp * a.gstride + col;
    *o = t;
  }
}

int colsum3_multi(const Colsum3Args* vs, int n, hipStream_t stream) {
  SERL_REQUIRE(n >= 1 && n <= kMaxColsum, "bad layer count %d", n);
  ColsumMulti mv{};
  int gx = 0, gy = 0;
  for (int i = 0; i < n; ++i) {
    mv.v[i] = vs[i];
    gx = std::max(gx, cdiv(vs[i].D, 64));
    gy = std::max(gy, vs[i].groups);
  }
  SERL_LAUNCH_CHAIN(colsum3_kernel, dim3(gx, gy, n), dim3(512), 0, stream, mv);
  SERL_HIP(hipGetLastError());
  return SERL_OK;
}

int colsum3(const float* dg, const float* xhat, const float* dpre, int groups, int rows_per_group, int D,
            float* o_gamma, float* o_beta, float* o_bias, long gstride, hipStream_t stream) {
  const Colsum3Args v{dg, xhat, dpre, groups, rows_per_group, D, o_gamma, o_beta, o_bias, gstride, 0};
  return colsum3_multi(&v, 1, stream);
}

// =============================================================================================
// SpatialLearnedEmbeddings (resnet_v1.py:94-111): f[n][c*F+j] = sum_hw x[n][hw][c]*K[hw][c][j]
// (+ Dropout(0.1) keep-mask, resnet_v1.py:351).  F == 8.
// =============================================================================================
__global__ __launch_bounds__(256) void sle_fwd_kernel(Multi<SleFwdArgs> mv, float keep_scale, int N, int HW, int Cc,
                                                     long xs, long ks, long ms, long fs) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)N * Cc) return;
  const SleFwdArgs& v = mv.v[blockIdx.z];  // blockIdx.z = instance, blockIdx.y = camera
  const float* x = v.x + blockIdx.y * xs;
  const float* K = v.K + blockIdx.y * ks;
  float* f = v.f + blockIdx.y * fs;
  const uint8_t* mask = v.mask ? v.mask + blockIdx.y * ms : nullptr;
  const int n = (int)(e / Cc), c = (int)(e - (long)n * Cc);
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 4
  for (int hw = 0; hw < HW; ++hw) {
    const float xv = x[((long)n * HW + hw) * Cc + c];
    const float4 k0 = *reinterpret_cast<const float4*>(K + ((long)hw * Cc + c) * 8);
    const float4 k1 = *reinterpret_cast<const float4*>(K + ((long)hw * Cc + c) * 8 + 4);
    acc[0] += xv * k0.x; acc[1] += xv * k0.y; acc[2] += xv * k0.z; acc[3] += xv * k0.w;
    acc[4] += xv * k1.x; acc[5] += xv * k1.y; acc[6] += xv * k1.z; acc[7] += xv * k1.w;
  }
  float* o = f + (long)n * Cc * 8 + (long)c * 8;
  if (mask) {
    const uint8_t* m = mask + (long)n * Cc * 8 + (long)c * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = m[j] ? acc[j] * keep_scale : 0.f;
  }
  *reinterpret_cast<float4*>(o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
  *reinterpret_cast<float4*>(o + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
}

int sle_fwd_multi(const SleFwdArgs* vs, int n, float keep_scale, int N, int HW, int Cc, int groups, long x_gs, long k_gs,
                  long mask_gs, long f_gs, hipStream_t stream) {
  SERL_REQUIRE(n >= 1 && n <= kMaxMulti, "bad instance count %d", n);
  Multi<SleFwdArgs> mv{};
  for (int i = 0; i < n; ++i) mv.v[i] = vs[i];
  SERL_LAUNCH_CHAIN(sle_fwd_kernel, dim3(cdiv((long)N * Cc, 256), groups, n), dim3(256), 0, stream, mv, keep_scale, N,
                     HW, Cc, x_gs, k_gs, mask_gs, f_gs);
  SERL_HIP(hipGetLastError());
  return SERL_OK;
}


// optional column copy riding along (the batch's actions into the critic input [enc | action]): ONE row by one wave, lane = column
__device__ __forceinline__ void copy_rider_row(const ProprioArgs& a, int row, int lane) {
  if (a.copy_dst && lane < a.copy_cols) a.copy_dst[(long)row * a.ld_copy_dst + lane] = a.copy_src[(long)row * a.ld_copy_src + lane];
}

// proprio branch (encoding.py:55-70) of ONE row by one wave, lane = output feature (also the body of proprio_fwd_kernel)
__device__ __forceinline__ void proprio_row(const ProprioArgs& a, int S, int row, int lane) {
  float v = a.b[lane];
  for (int s0 = 0; s0 < S; s0 += 64) {  // the state row travels once, coalesced, and is broadcast lane by lane
    const float mine = (s0 + lane < S) ? a.state[(long)row * S + s0 + lane] : 0.f;
    const int cnt = min(64, S - s0);
    int s = 0;
    for (; s + 8 <= cnt; s += 8) {
      float w[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) w[j] = a.W[(s0 + s + j) * 64 + lane];
#pragma unroll
      for (int j = 0; j < 8; ++j) v += __shfl(mine, s + j) * w[j];
    }
    for (; s < cnt; ++s) v += __shfl(mine, s) * a.W[(s0 + s) * 64 + lane];
  }
  float s1 = v, s2 = v * v;
  wave_sum2(s1, s2);
  float mean, rstd;
  ln_mean_rstd<64>(s1, s2, mean, rstd);
  const float xh = (v - mean) * rstd;
  a.y[(long)row * a.ld_y + lane] = tanhf(xh * a.gamma[lane] + a.beta[lane]);
  if (a.xhat) a.xhat[(long)row * 64 + lane] = xh;
  if (a.rstd && lane == 0) a.rstd[row] = rstd;
  copy_rider_row(a, row, lane);
}

// SpatialLearnedEmbeddings, channel-blocked: a workgroup = 256 channels x kSleNb samples.  The embedding kernel K
// ([HW][C][8]: 256 KB per camera at 4x4x512) is read ONCE per workgroup, kPx pixels at a time into registers, instead of
// once per sample (round 3: 393 MB of L2 reads per update phase, 30 us alone / 160-190 us next to the trunk pass); every
// sample's 8 outputs stay in registers across the pixel loop (same hw-ascending sum as before: bit-identical).  The Dropout(0.1)
// keep-mask (resnet_v1.py:351), when not supplied, is hashed from (seed, camera, GLOBAL sample, channel): three 64-bit hashes
// give the eight 24-bit uniforms of a thread's eight outputs -- no mask tensor, no gen_noise launch.  Workgroups past the SLE
// range run the proprio branch of the same instance (camera 0 only): one launch instead of two.  has_proprio == 2 (an agent
// without the proprio branch, use_proprio=False): those workgroups carry the instance's column-copy rider alone.
// kSleNb samples per workgroup; a rank's share of a data-parallel batch (<= 64 samples) takes 2 samples x 4 pixels (64 VGPRs), which
// keeps more workgroups in flight (96 workgroups of 8 samples each took 64 us next to the trunk pass at 32 samples).  Larger
// batches take 4 samples x 2 pixels: 32 sums + 16 embedding values + 8 pixels = 62 VGPRs, so a wave fits into the 80 registers per
// SIMD that two resident trunk workgroups leave (scripts/kernel_resources.py).  The 8 x 4 form this replaces took 150 and fitted
// beside no trunk kernel; alone it was no faster (31 / 37 us per launch at B = 256 against 26 / 34, profiles/README.md).
template <int kSleNb, int kPx>
__global__ __launch_bounds__(256) void sle_proprio_fwd_kernel(Multi<SleFwdArgs> mv, Multi<ProprioArgs> pv, int has_proprio,
                                                              float keep_scale, unsigned keep_thr, float keep_p, int N, int HW, int Cc,
                                                              long xs, long ks, long ms, long fs, int S, int nb_sle) {
  if ((int)blockIdx.x >= nb_sle) {
    if (!has_proprio || blockIdx.y != 0) return;
    const int row = ((int)blockIdx.x - nb_sle) * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    if (has_proprio == 2) copy_rider_row(pv.v[blockIdx.z], row, threadIdx.x & 63);
    else proprio_row(pv.v[blockIdx.z], S, row, threadIdx.x & 63);
    return;
  }
  const SleFwdArgs& v = mv.v[blockIdx.z];  // blockIdx.z = instance, blockIdx.y = camera
  const int cblocks = (Cc + 255) / 256;
  const int c = ((int)blockIdx.x % cblocks) * 256 + threadIdx.x, n0 = ((int)blockIdx.x / cblocks) * kSleNb;
  if (c >= Cc) return;
  const float* x = v.x + blockIdx.y * xs + (long)n0 * HW * Cc + c;
  const float* K = v.K + blockIdx.y * ks + (long)c * 8;
  const int ns = min(kSleNb, N - n0);
  float acc[kSleNb][8];
#pragma unroll
  for (int s = 0; s < kSleNb; ++s)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[s][j] = 0.f;
  for (int hw0 = 0; hw0 < HW; hw0 += kPx) {
    float4 k0[kPx], k1[kPx];
#pragma unroll
    for (int i = 0; i < kPx; ++i) {
      const int hw = min(hw0 + i, HW - 1);
      k0[i] = *reinterpret_cast<const float4*>(K + (long)hw * Cc * 8);
      k1[i] = *reinterpret_cast<const float4*>(K + (long)hw * Cc * 8 + 4);
    }
    // (no branch on the sample count: samples past the end re-read the last one and are never stored -- a branch per sample kept
    //  the compiler from issuing the 32 pixel loads of a chunk together: 48 us against 36 for the un-blocked kernel)
    float xv[kSleNb][kPx];
#pragma unroll
    for (int s = 0; s < kSleNb; ++s)
#pragma unroll
      for (int i = 0; i < kPx; ++i) xv[s][i] = x[((long)min(s, ns - 1) * HW + min(hw0 + i, HW - 1)) * Cc];
#pragma unroll
    for (int i = 0; i < kPx; ++i) {
      if (hw0 + i < HW) {   // (uniform; pixels past HW must not touch the sums)
#pragma unroll
        for (int s = 0; s < kSleNb; ++s) {
          acc[s][0] += xv[s][i] * k0[i].x; acc[s][1] += xv[s][i] * k0[i].y; acc[s][2] += xv[s][i] * k0[i].z; acc[s][3] += xv[s][i] * k0[i].w;
          acc[s][4] += xv[s][i] * k1[i].x; acc[s][5] += xv[s][i] * k1[i].y; acc[s][6] += xv[s][i] * k1[i].z; acc[s][7] += xv[s][i] * k1[i].w;
        }
      }
    }
  }
  float* f = v.f + blockIdx.y * fs + (long)n0 * Cc * 8 + (long)c * 8;
  const uint8_t* mask = v.mask ? v.mask + blockIdx.y * ms + (long)n0 * Cc * 8 + (long)c * 8 : nullptr;
#pragma unroll
  for (int s = 0; s < kSleNb; ++s) {
    if (s >= ns) break;
    if (mask) {
      const uint8_t* m = mask + (long)s * Cc * 8;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[s][j] = m[j] ? acc[s][j] * keep_scale : 0.f;
    } else if (v.gen == 2) {   // jax.random.bernoulli(key of this camera, keep, (rows, Cc * 8)): element (row, c * 8 + j)
      const uint32_t k0 = v.tf_key[blockIdx.y][0], k1 = v.tf_key[blockIdx.y][1];
      const uint64_t rowlen = (uint64_t)Cc * 8ull, total = (uint64_t)v.tf_rows * rowlen;
      const uint64_t e0 = (uint64_t)(v.tf_row0 + n0 + s) * rowlen + (uint64_t)c * 8ull;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        acc[s][j] = bits_to_unit(random_bits_at(k0, k1, total, e0 + (uint64_t)j)) < keep_p ? acc[s][j] * keep_scale : 0.f;
    } else if (v.gen) {
      const uint64_t ctr = (((uint64_t)blockIdx.y * (uint64_t)v.rows_global + (uint64_t)(v.row_offset + n0 + s)) * (uint64_t)Cc + (uint64_t)c) * 3ull;
      const uint64_t h0 = mix64(v.seed ^ mix64(ctr)), h1 = mix64(v.seed ^ mix64(ctr + 1)), h2 = mix64(v.seed ^ mix64(ctr + 2));
      const unsigned u[8] = {(unsigned)(h0 & 0xFFFFFF), (unsigned)((h0 >> 24) & 0xFFFFFF), (unsigned)((h0 >> 48) | ((h1 & 0xFF) << 16)),
                             (unsigned)((h1 >> 8) & 0xFFFFFF), (unsigned)((h1 >> 32) & 0xFFFFFF), (unsigned)((h1 >> 56) | ((h2 & 0xFFFF) << 8)),
                             (unsigned)((h2 >> 16) & 0xFFFFFF), (unsigned)(h2 >> 40)};
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[s][j] = u[j] < keep_thr ? acc[s][j] * keep_scale : 0.f;
    }
    *reinterpret_cast<float4*>(f + (long)s * Cc * 8) = make_float4(acc[s][0], acc[s][1], acc[s][2], acc[s][3]);
    *reinterpret_cast<float4*>(f + (long)s * Cc * 8 + 4) = make_float4(acc[s][4], acc[s][5], acc[s][6], acc[s][7]);
  }
}

int sle_proprio_fwd_multi(const SleFwdArgs* vs, const ProprioArgs* ps, int n, float keep, int N, int HW, int Cc, int groups, long x_gs,
                          long k_gs, long mask_gs, long f_gs, int state_dim, hipStream_t stream) {
  SERL_REQUIRE(n >= 1 && n <= kMaxMulti, "bad instance count %d", n);
  Multi<SleFwdArgs> mv{};
  Multi<ProprioArgs> pv{};
  for (int i = 0; i < n; ++i) {
    mv.v[i] = vs[i];
    if (ps) { pv.v[i] = ps[i]; SERL_REQUIRE(!ps[i].copy_dst || ps[i].copy_cols <= 64, "copy_cols > 64"); }
  }
  // (block sizes: see the kernel; tests/test_sle_block_gpu.py holds its row counts to the 4)
  const int nb = N <= 64 ? 2 : 4;
  const int nb_sle = cdiv(Cc, 256) * cdiv(N, nb), nb_prop = ps ? cdiv(N, 4) : 0;
  // ps without a state: no proprio rows, the trailing workgroups carry the riders alone (the caller passes none without a rider)
  const int has_prop = !ps ? 0 : (ps[0].state ? 1 : 2);
  for (int i = 0; ps && i < n; ++i) SERL_REQUIRE((ps[i].state != nullptr) == (has_prop == 1), "proprio rows in some instances of a launch and not in others");
  if (nb == 2)
    SERL_LAUNCH_CHAIN((sle_proprio_fwd_kernel<2, 4>), dim3(nb_sle + nb_prop, groups, n), dim3(256), 0, stream, mv, pv, has_prop,
                      1.0f / keep, (unsigned)(keep * 16777216.0f), keep, N, HW, Cc, x_gs, k_gs, mask_gs, f_gs, state_dim, nb_sle);
  else
    SERL_LAUNCH_CHAIN((sle_proprio_fwd_kernel<4, 2>), dim3(nb_sle + nb_prop, groups, n), dim3(256), 0, stream, mv, pv, has_prop,
                      1.0f / keep, (unsigned)(keep * 16777216.0f), keep, N, HW, Cc, x_gs, k_gs, mask_gs, f_gs, state_dim, nb_sle);
  SERL_HIP(hipGetLastError());
  return SERL_OK;
}

// dK partial[split][hw][c][j] = sum_{n in split} x[n][hw][c] * df[n][c*8+j]
__global__ __launch_bounds__(256) void sle_bwd_kernel(const float* x, const float* df, float* partial, int N,
                                                     int HW, int Cc, int nsplit, long x_gs, long df_gs, long part_gs) {
  const int c = blockIdx.x * 256 + threadIdx.x, hw = blockIdx.y, sp = blockIdx.z % nsplit, grp = blockIdx.z / nsplit;
  if (c >= Cc) return;
  x += grp * x_gs; df += grp * df_gs; partial += grp * part_gs;  // grp = camera
  const int per = (N + nsplit - 1) / nsplit;
  const int nb = sp * per, ne = min(N, nb + per);
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int n = nb; n < ne; ++n) {
    const float xv = x[((long)n * HW + hw) * Cc + c];
    const float4 d0 = *reinterpret_cast<const float4*>(df + (long)n * Cc * 8 + (long)c * 8);
    const float4 d1 = *reinterpret_cast<const float4*>(df + (long)n * Cc * 8 + (long)c * 8 + 4);
    acc[0] += xv * d0.x; acc[1] += xv * d0.y; acc[2] += xv * d0.z; acc[3] += xv * d0.w;
    acc[4] += xv * d1.x; acc[5] += xv * d1.y; acc[6] += xv * d1.z; acc[7] += xv * d1.w;
  }
  float* o = partial + (((long)sp * HW + hw) * Cc + c) * 8;
  *reinterpret_cast<float4*>(o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
  *reinterpret_cast<float4*>(o + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
}

// the same partial sums, then the sum over the batch splits by the LAST workgroup to arrive at its (camera, pixel, channel
// block) -- see "last-arriver epilogues" above: sc1 partial stores, drain, ticket; sc1 loads in split order on the reducer
__global__ __launch_bounds__(256) void sle_bwd_fused_kernel(const float* x, const float* df, float* partial, int N, int HW, int Cc,
                                                           int nsplit, long x_gs, long df_gs, long part_gs, float* out, long out_gs,
                                                           int* ctr) {
  __shared__ int s_last;
  const int c = blockIdx.x * 256 + threadIdx.x, hw = blockIdx.y, sp = blockIdx.z % nsplit, grp = blockIdx.z / nsplit;
  x += grp * x_gs; df += grp * df_gs; partial += grp * part_gs;  // grp = camera
  const int per = (N + nsplit - 1) / nsplit;
  const int nb = sp * per, ne = min(N, nb + per);
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (c < Cc) {
    for (int n = nb; n < ne; ++n) {
      const float xv = x[((long)n * HW + hw) * Cc + c];
      const float4 d0 = *reinterpret_cast<const float4*>(df + (long)n * Cc * 8 + (long)c * 8);
      const float4 d1 = *reinterpret_cast<const float4*>(df + (long)n * Cc * 8 + (long)c * 8 + 4);
      acc[0] += xv * d0.x; acc[1] += xv * d0.y; acc[2] += xv * d0.z; acc[3] += xv * d0.w;
      acc[4] += xv * d1.x; acc[5] += xv * d1.y; acc[6] += xv * d1.z; acc[7] += xv * d1.w;
    }
    const __amdgpu_buffer_rsrc_t rs = rsrc_of(partial);
    const long o = (((long)sp * HW + hw) * Cc + c) * 8;
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, (f32x4){acc[0], acc[1], acc[2], acc[3]}), rs, (int)(o * 4), 0, kSc1);
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, (f32x4){acc[4], acc[5], acc[6], acc[7]}), rs, (int)(o * 4 + 16), 0, kSc1);
  }
  if (!arrive_is_last(ctr + ((long)grp * HW + hw) * gridDim.x + blockIdx.x, nsplit, &s_last)) return;
  if (c >= Cc) return;
  const __amdgpu_buffer_rsrc_t rs = rsrc_of(partial);
  f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < nsplit; ++s) {
    const long o = (((long)s * HW + hw) * Cc + c) * 8;
    s0 += ld_sc1(rs, o);
    s1 += ld_sc1(rs, o + 4);
  }
  float* o = out + grp * out_gs + ((long)hw * Cc + c) * 8;
  *reinterpret_cast<f32x4*>(o) = s0;
  *reinterpret_cast<f32x4*>(o + 4) = s1;
}

int sle_bwd_fused(const float* x, const float* df, float* partial, int N, int HW, int Cc, int nsplit, int groups,
                  long x_gs, long df_gs, long part_gs, float* out, long out_gs, int* ctr, hipStream_t stream) {
  SERL_REQUIRE((long)nsplit * HW * Cc * 8 * 4 < (1L << 31), "SLE partial sums exceed 2 GB");
  SERL_LAUNCH_CHAIN(sle_bwd_fused_kernel, dim3(cdiv(Cc, 256), HW, nsplit * groups), dim3(256), 0, stream, x, df, partial, N,
                     HW, Cc, nsplit, x_gs, df_gs, part_gs, out, out_gs, ctr);
  SERL_HIP(hipGetLastError());
  return SERL_OK;
}

int sle_bwd(const float* x, const float* df, float* partial, int N, int HW, int Cc, int nsplit, int groups,
            long x_gs, long df_gs, long part_gs, hipStream_t stream) {
  SERL_LAUNCH_CHAIN(sle_bwd_kernel, dim3(cdiv(Cc, 256), HW, nsplit * groups), dim3(256), 0, stream, x, df, partial, N,
                     HW, Cc, nsplit, x_gs, df_gs, part_gs);
  SERL_HIP(hipGetLastError());
  return SERL_OK;
}

// =============================================================================================
// REDQ target + critic loss (sac.py:142-191).  Single workgroup: deterministic reductions.
//   y[b] = r[b] + discount*mask[b]*min(Qt[i0][b], Qt[i1][b]);  dQ = 2(Q-y)/(E*Bg)
//   scalars[0..2] = sum (Q-y)^2, sum Q, sum y   (local sums; the host / all-reduce normalises)
//   dhead_b = sum dQ  (gradient of the shared head bias)
// =============================================================================================
__global__ __launch_bounds__(256) void critic_loss_kernel(LossArgs L) {
  __shared__ float red[4][256];
  critic_loss_body(L, red);
}

int critic_loss(const float* qt, const float* q, const float* reward, const float* mask, RedqSel sel, int E,
                int B, float discount, float inv_norm, float* y_out, float* dq, float* scalars, float* dbias,
                hipStream_t stream, bool per_member_bias, const float* logp_next, const float* alpha) {
  SERL_REQUIRE(!per_member_bias || E <= 16, "per-member head bias supports ensembles of at most 16 (got %d)", E);
  SERL_REQUIRE(sel.n >= 0 && sel.n <= 16, "critic_subsample_size %d not in [0, 16]", sel.n);
  const LossArgs L{1, qt, q, reward, mask, sel, E, B, discount, inv_norm, y_out, dq, scalars, dbias, per_member_bias ? 1 : 0, logp_next, alpha};
  SERL_LAUNCH_CHAIN(critic_loss_kernel, dim3(1), dim3(256), 0, stream, L);
  SERL_HIP(hipGetLastError());
  return SERL_OK;
}

// =============================================================================================
// Gaussian policy head (actor_critic_nets.py:179-272, distrax MultivariateNormalDiag [+ Tanh])
//   std = clip(exp(log_std), std_min, std_max); u = mean + std*eps; a = tanh(u)
//   logp = sum_j(-eps^2/2 - log std - log(2pi)/2) - sum_j 2(log2 - u - softplus(-2u))
// pre: [2][B][A] (mean slab, log_std slab; biases already added).  MODE: see policy_dist_rows (kPolSoftplus: std from
// softplus; kPolUniform: log_std = bias_ls for every row, one slab group; kPolFixed: std = clip(bias_ls), one slab group, pre is
// [1][B][A]; kPolNoTanh: a = u and no second sum)
// =============================================================================================
template <int MODE>
__global__ void policy_dist_fwd_kernel(Multi<PolicyDistArgs> mv, int B, int A, float std_min, float std_max) {
  const PolicyDistArgs& v = mv.v[blockIdx.x];  // one workgroup per instance
  __shared__ float red[256];
  float local = 0.f;
  for (int b = threadIdx.x; b < B; b += 256) {
    float lp = 0.f;
    for (int j = 0; j < A; ++j) {
      float mean = v.bias_mean[j], ls = v.bias_ls[j];
      for (int sp = 0; sp < v.S; ++sp) {  // K-split slabs of the head GEMM: [mean | log_std][split][B][A]
        mean += v.slabs[((long)sp * B + b) * A + j];
        if (policy_ls_group<MODE>()) ls += v.slabs[(((long)v.S + sp) * B + b) * A + j];
      }
      const float e = v.eps[(long)b * A + j];
      v.pre[(long)b * A + j] = mean;
      if (!policy_fixed<MODE>()) v.pre[((long)B + b) * A + j] = ls;
      const float sd = policy_std<MODE>(ls, std_min, std_max);
      const float u = mean + sd * e;
      v.act[(long)b * v.ld_act + j] = (MODE & kPolNoTanh) ? u : tanhf(u);
      v.std_out[(long)b * A + j] = sd;
      lp += -0.5f * e * e - logf(sd) - 0.91893853320467274f;
      if (!(MODE & kPolNoTanh)) lp -= 2.f * (0.69314718055994531f - u - softplusf(-2.f * u));
    }
    v.logp[b] = lp;
    local += lp;
  }
  red[threadIdx.x] = local;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0 && v.sum_logp) *v.sum_logp = red[0];
  if (threadIdx.x == 0 && v.alpha_out) v.alpha_out[0] = softplusf(v.lam[0]);
}

int policy_dist_fwd_multi(const PolicyDistArgs* vs, int n, int B, int A, float std_min, float std_max, hipStream_t stream) {
  SERL_REQUIRE(n >= 1 && n <= kMaxMulti, "bad instance count %d", n);
  Multi<PolicyDistArgs> mv{};
  for (int i = 0; i < n; ++i) {
    mv.v[i] = vs[i];
    SERL_REQUIRE(vs[i].mode == vs[0].mode, "the policy heads of one launch share a distribution mode");
  }
#define SERL_X(M) SERL_LAUNCH_CHAIN(policy_dist_fwd_kernel<M>, dim3(n), dim3(256), 0, stream, mv, B, A, std_min, std_max)
  SERL_POLICY_MODE_SWITCH(vs[0].mode, SERL_X, SERL_REQUIRE(false, "bad policy distribution mode %d", vs[0].mode))
#undef SERL_X
  SERL_HIP(hipGetLastError());
  return SERL_OK;
}

// =============================================================================================
// The policy distribution itself, for inspection (forward_policy(obs, train=False), sac.py:71-91): no sample is drawn.
//   mean = loc (pre-squash);  std = scale_diag, by the expressions of policy_dist_fwd_kernel (same bits);  mode = tanh(mean), or
//   mean with kPolNoTanh;  logp[row] = log pi(act[row] | s) when `act` is given:
//     kPolNoTanh:  sum_j log N(a_j; mean_j, std_j)
//     else (distrax Transformed.log_prob under the Tanh bijector):  u = atanh(a) = (log1p(a) - log1p(-a)) / 2,
//                  sum_j [log N(u_j; mean_j, std_j) - 2 (log 2 - u_j - softplus(-2 u_j))]
//   softplus(-2u) = max(-2u, 0) + log1p(exp(-|2u|)): the exponent is never positive, nothing overflows at any finite u.
// An action component with |a_j| >= 1 has no finite pre-image: u_j = +-inf (or NaN beyond) and the row's logp is not finite, as
// the reference's is -- it is NOT clamped (stored gripper commands of exactly +-1 are common: clip them before asking).
// One wave owns one row and lane j holds action column j (A <= 64; a lane past A reads column 0 and contributes 0), so the sum
// over the row is the xor butterfly of wave_sum2: a fixed order that depends on neither the grid nor the row count.  Loads are
// issued together on clamped addresses before any store; no LDS, no scratch.
// =============================================================================================
template <int MODE>
__global__ __launch_bounds__(256) void policy_stats_kernel(PolicyStatsArgs v) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= v.rows) return;   // (uniform over the wave)
  const int A = v.A;
  const bool live = lane < A;
  const int j = live ? lane : 0;
  const long e = (long)row * A + j;
  float mean = v.bias_mean[j], ls = v.bias_ls[j];
  const float a = v.act ? v.act[e] : 0.f;
  for (int sp = 0; sp < v.S; ++sp) {   // K-split slabs of the head GEMM, [mean | log_std][split][rows][A], added in index order
    mean += v.slabs[((long)sp * v.rows) * A + e];
    if ((MODE & kPolStdMask) != kPolUniform) ls += v.slabs[(((long)v.S + sp) * v.rows) * A + e];
  }
  const float sd = fminf(fmaxf(policy_std_raw<MODE>(ls), v.std_min), v.std_max);
  float lp = 0.f;
  if (v.logp) {   // (uniform: a launch argument)
    float u = a;
    if (!(MODE & kPolNoTanh)) u = 0.5f * (log1pf(a) - log1pf(-a));
    const float z = (u - mean) / sd;
    lp = -0.5f * z * z - logf(sd) - 0.91893853320467274f;
    if (!(MODE & kPolNoTanh)) lp -= 2.f * (0.69314718055994531f - u - softplusf(-2.f * u));
    lp = live ? lp : 0.f;
    float unused = 0.f;
    wave_sum2(lp, unused);
  }
  if (live) {
    if (v.mean) v.mean[e] = mean;
    if (v.std) v.std[e] = sd;
    if (v.mode_out) v.mode_out[e] = (MODE & kPolNoTanh) ? mean : tanhf(mean);
  }
  if (v.logp && lane == 0) v.logp[row] = lp;
}
// kPolFixed: the same row with std = clip(fixed_std[j]) -- bias_ls is the agent's fixed_std vector, read like the biases (a lane past A
// reads column 0) and before any store; one slab group, no exp.  Kernels of their own: the six above keep their text.
template <bool NOTANH>
__global__ __launch_bounds__(256) void policy_stats_fixed_kernel(PolicyStatsArgs v) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= v.rows) return;   // (uniform over the wave)
  const int A = v.A;
  const bool live = lane < A;
  const int j = live ? lane : 0;
  const long e = (long)row * A + j;
  float mean = v.bias_mean[j];
  const float fixed = v.bias_ls[j];
  const float a = v.act ? v.act[e] : 0.f;
  for (int sp = 0; sp < v.S; ++sp) mean += v.slabs[((long)sp * v.rows) * A + e];   // K-split slabs of the mean's group, in index order
  const float sd = policy_std<kPolFixed>(fixed, v.std_min, v.std_max);
  float lp = 0.f;
  if (v.logp) {   // (uniform: a launch argument)
    float u = a;
    if (!NOTANH) u = 0.5f * (log1pf(a) - log1pf(-a));
    const float z = (u - mean) / sd;
    lp = -0.5f * z * z - logf(sd) - 0.91893853320467274f;
    if (!NOTANH) lp -= 2.f * (0.69314718055994531f - u - softplusf(-2.f * u));
    lp = live ? lp : 0.f;
    float unused = 0.f;
    wave_sum2(lp, unused);
  }
  if (live) {
    if (v.mean) v.mean[e] = mean;
    if (v.std) v.std[e] = sd;
    if (v.mode_out) v.mode_out[e] = NOTANH ? mean : tanhf(mean);
  }
  if (v.logp && lane == 0) v.logp[row] = lp;
}

int policy_stats(const PolicyStatsArgs& v, hipStream_t stream) {
  SERL_REQUIRE(v.rows >= 1 && v.A >= 1 && v.A <= 64, "policy statistics: %d rows x %d action columns (one lane per column: at most 64)", v.rows, v.A);
  SERL_REQUIRE(!v.logp || v.act, "policy statistics: a log-density needs the actions it is the density of");
#define SERL_X(M) SERL_LAUNCH_CHAIN(policy_stats_kernel<M>, dim3(cdiv(v.rows, 4)), dim3(256), 0, stream, v)
  switch (v.mode) {
    SERL_POLICY_PARAM_CASES(SERL_X)
    case kPolFixed: SERL_LAUNCH_CHAIN(policy_stats_fixed_kernel<false>, dim3(cdiv(v.rows, 4)), dim3(256), 0, stream, v); break;
    case kPolFixed | kPolNoTanh: SERL_LAUNCH_CHAIN(policy_stats_fixed_kernel<true>, dim3(cdiv(v.rows, 4)), dim3(256), 0, stream, v); break;
    default: SERL_REQUIRE(false, "bad policy distribution mode %d", v.mode);
  }
#undef SERL_X
  SERL_HIP(hipGetLastError());
  return SERL_OK;
}


// proprio branch (encoding.py:55-70): y = tanh(LayerNorm_1e-6(state W + b)), W [S][64]; one wave per row,
// lane = output feature.  Replaces a GEMM + LN launch pair for this tiny layer.
__global__ __launch_bounds__(256) void proprio_fwd_kernel(Multi<ProprioArgs> mv, int S, int rows) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row < rows) proprio_row(mv.v[blockIdx.y], S, row, threadIdx.x & 63);
}

int proprio_fwd_multi(const ProprioArgs* vs, int n, int S, int rows, hipStream_t stream) {
  SERL_REQUIRE(n >= 1 && n <= kMaxMulti, "bad instance count %d", n);
  Multi<ProprioArgs> mv{};
  for (int i = 0; i < n; ++i) {
    mv.v[i] = vs[i];
    SERL_REQUIRE(!vs[i].copy_dst || vs[i].copy_cols <= 64, "copy_cols > 64");
  }
  SERL_LAUNCH_CHAIN(proprio_fwd_kernel, dim3(cdiv(rows, 4), n), dim3(256), 0, stream, mv, S, rows);
  SERL_HIP(hipGetLastError());
  return SERL_OK;
}


// backward of the actor loss through the distribution:
//   G_u = dL/da*(1-a^2) + c_lp*2a   (d logp/du = 2 tanh u);  dmean = G_u;
//   dstd = G_u*eps - c_lp/std;  dlog_std = dstd*std if std_min < exp(ls) < std_max else 0
// dpre: [2][B][A].  c_lp = dL/dlogp (device scalar *alpha times coef).
// MODE (see policy_dist_rows): kPolNoTanh: G_u = dL/da; kPolSoftplus: dlog_std = dstd * sigmoid(ls) under the same gate on
// softplus(ls); kPolUniform: ls is the shared log_stds vector (as the forward left it in pre) and the column sums of the second
// slab -- the sums that make the log-std bias gradient -- are the gradient of log_stds.  kPolFixed: the std has no parameter:
// dpre is [1][B][A] = G_u alone, and pre's second half, stdv and eps are not read.
template <int MODE>
__global__ void policy_dist_bwd_kernel(const float* da, long ld_da, const float* act, long ld_act,
                                       const float* pre, const float* stdv, const float* eps,
                                       const float* alpha, float coef, int B, int A, float std_min,
                                       float std_max, float* dpre, const float* q, int E, float* qmean_out) {
  if (blockIdx.x == gridDim.x - 1) {  // rider (one extra workgroup): sum_b mean_e Q[e][b], the actor-loss info scalar
    __shared__ float red[256];
    float sacc = 0.f;
    for (int b = threadIdx.x; b < B; b += 256) {
      float m = 0.f;
      for (int e = 0; e < E; ++e) m += q[(long)e * B + b];
      sacc += m / (float)E;
    }
    red[threadIdx.x] = sacc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
      __syncthreads();
    }
    if (threadIdx.x == 0) qmean_out[0] = red[0];
    return;
  }
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= B * A) return;
  const int b = e / A, j = e - b * A;
  const float c_lp = alpha[0] * coef;
  float gu = da[(long)b * ld_da + j];
  if (!(MODE & kPolNoTanh)) {
    const float a = act[(long)b * ld_act + j];
    gu = gu * (1.f - a * a) + c_lp * 2.f * a;
  }
  if (policy_fixed<MODE>()) {
    dpre[e] = gu;
    return;
  }
  const float sd = stdv[e];
  const float ls = pre[((long)B + b) * A + j];
  const float raw = policy_std_raw<MODE>(ls);
  const float dstd = gu * eps[e] - c_lp / sd;
  dpre[e] = gu;
  const float draw = (MODE & kPolStdMask) == kPolSoftplus ? 1.f / (1.f + expf(-ls)) : sd;   // d raw / d ls (exp: raw == sd inside the clip)
  dpre[(long)B * A + e] = (raw > std_min && raw < std_max) ? dstd * draw : 0.f;
}

int policy_dist_bwd(const float* da, long ld_da, const float* act, long ld_act, const float* pre,
                    const float* stdv, const float* eps, const float* alpha, float coef, int B, int A,
                    float std_min, float std_max, float* dpre, const float* q, int E, float* qmean_out,
                    hipStream_t stream, int mode) {
#define SERL_X(M)                                                                                                            \
  SERL_LAUNCH_CHAIN(policy_dist_bwd_kernel<M>, dim3(cdiv(B * A, 256) + 1), dim3(256), 0, stream, da, ld_da, act, ld_act, pre, \
                    stdv, eps, alpha, coef, B, A, std_min, std_max, dpre, q, E, qmean_out)
  SERL_POLICY_MODE_SWITCH(mode, SERL_X, SERL_REQUIRE(false, "bad policy distribution mode %d", mode))
#undef SERL_X
  SERL_HIP(hipGetLastError());
  return SERL_OK;
}

// small helpers ---------------------------------------------------------------------------------
__global__ void copy_cols_multi_kernel(Multi<CopyJob> mv, int rows) {
  const CopyJob& j = mv.v[blockIdx.y];
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= rows * j.cols) return;
  const int r = e / j.cols, c = e - r * j.cols;
  j.dst[(long)r * j.ld_dst + c] = j.src[(long)r * j.ld_src + c];
}
int copy_cols_multi(const CopyJob* jobs, int n, int rows, hipStream_t stream) {
  SERL_REQUIRE(n >= 1 && n <= kMaxMulti, "bad job count %d", n);
  Multi<CopyJob> mv{};
  int cmax = 0;
  for (int i = 0; i < n; ++i) { mv.v[i] = jobs[i]; cmax = std::max(cmax, jobs[i].cols); }
  SERL_LAUNCH_CHAIN(copy_cols_multi_kernel, dim3(cdiv((long)rows * cmax, 256), n), dim3(256), 0, stream, mv, rows);
  SERL_HIP(hipGetLastError());
  return SERL_OK;
}

__global__ void fill_kernel(float* p, float v, long n) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e < n) p[e] = v;
}
int fill(float* p, float v, long n, hipStream_t stream) {
  SERL_LAUNCH_CHAIN(fill_kernel, dim3(cdiv(n, 256)), dim3(256), 0, stream, p, v, n);
  SERL_HIP(hipGetLastError());
  return SERL_OK;
}

// =============================================================================================
// 3x Adam over the full tree (restricted to each optimizer's non-zero support) + summed update +
// target EMA.  common.py:124-168, optimizers.py:32-46, optax.adam(b1 .9, b2 .999, eps 1e-8).
// A tx that is not in networks_to_update still steps with g = 0 (sac.py:276-277): its moments
// decay and its momentum keeps moving the parameters.
// =============================================================================================
// one element: the frozen leaves past P, the temperature at P - 1, everything a 4-wide vector cannot take
__device__ __forceinline__ void adam_elem(const AdamArgs& a, long i, float cs_c, float cs_a) {
  // adamw (optimizers.py:39-42): every optimizer with a weight decay adds -lr*wd*p on EVERY leaf of the tree
  const float wd_total = a.lr_c * a.wd_c + a.lr_a * a.wd_a + a.lr_t * a.wd_t;
  if (i >= a.P) {  // frozen-trunk leaves: no gradient ever reaches them; weight decay and the target EMA still do
    const long k = i - a.P;
    if (k < a.n_frozen) {
      float p = a.frozen[k];
      if (wd_total != 0.f) { p -= wd_total * p; a.frozen[k] = p; }
      if (a.ema_on) a.frozen_target[k] = p * a.tau + a.frozen_target[k] * (1.f - a.tau);
    }
    return;
  }
  const float b1 = 0.9f, b2 = 0.999f, eps = 1e-8f;
  const float p0 = a.theta[i];
  float ua = 0.f, uc = 0.f, ut = 0.f;
  if (i < a.Pc) {
    const float g = a.critic_on ? a.g_critic[i] * cs_c : 0.f;
    const float m = b1 * a.m_c[i] + (1.f - b1) * g;
    const float v = b2 * a.v_c[i] + (1.f - b2) * g * g;
    a.m_c[i] = m; a.v_c[i] = v;
    uc = -a.lr_c * (m / a.bc1) / (sqrtf(v / a.bc2) + eps);
  }
  if (i >= a.Pa0 && i < a.Pa1) {
    const long k = i - a.Pa0;
    const float g = a.actor_on ? a.g_actor[k] * cs_a : 0.f;
    const float m = b1 * a.m_a[k] + (1.f - b1) * g;
    const float v = b2 * a.v_a[k] + (1.f - b2) * g * g;
    a.m_a[k] = m; a.v_a[k] = v;
    ua = -a.lr_a * (m / a.bc1) / (sqrtf(v / a.bc2) + eps);
  }
  if (i == a.P - 1) {  // temperature multiplier (lagrange.py): dL/dlambda = sigmoid(lambda)*(H - H_target)
    float g = 0.f;
    if (a.temp_on) {
      const float H = -a.sum_logp_next[0] * a.inv_batch;
      g = (1.f / (1.f + expf(-p0))) * (H - a.target_entropy);
      a.temp_grad_out[0] = g;
      if (a.clip_t > 0.f && !(fabsf(g) < a.clip_t)) g = g * a.clip_t / fabsf(g);
    }
    const float m = b1 * a.m_t[0] + (1.f - b1) * g;
    const float v = b2 * a.v_t[0] + (1.f - b2) * g * g;
    a.m_t[0] = m; a.v_t[0] = v;
    ut = -a.lr_t * (m / a.bc1) / (sqrtf(v / a.bc2) + eps);
  }
  // optax.adamw: -lr * (adam direction + wd * p); the three optimizers' updates are summed (common.py:161-164)
  if (a.wd_a != 0.f) ua -= a.lr_a * a.wd_a * p0;
  if (a.wd_c != 0.f) uc -= a.lr_c * a.wd_c * p0;
  if (a.wd_t != 0.f) ut -= a.lr_t * a.wd_t * p0;
  const float p = p0 + ((ua + uc) + ut);
  a.theta[i] = p;
  if (a.ema_on) a.theta_target[i] = p * a.tau + a.theta_target[i] * (1.f - a.tau);
}

// A thread owns FOUR consecutive leaves.  A vector that lies wholly inside or outside each optimizer's support (and does not
// hold the temperature) takes the fast path: its eight 16-byte loads are issued together, unconditionally (a vector outside a
// support reads the support's first elements and ignores them), then the arithmetic of adam_elem per element, then the stores.
// The one-leaf-per-thread kernel of rounds 1-3 put every 4-byte load into its own exec-masked region behind stores that were
// still in flight (one vmcnt for both): four dependent round trips per thread, 45 us for the critic step.
__global__ __launch_bounds__(256) void adam_ema_kernel(AdamArgs a) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t == 0 && a.info_mode) {  // info dict of this step (riding along: one launch less on the chain)
    const float* sc = a.scalars;
    float* acc = a.info_acc;
    if (a.info_mode & 1) {  // critic step (sac.py:118-191); weighted mean over UTD minibatches
      if (a.info_reset)
        for (int k = 0; k < 8; ++k) acc[k] = 0.f;
      acc[0] += a.info_w * sc[0] * a.inv_eb;   // critic_loss
      acc[1] += a.info_w * sc[1] * a.inv_eb;   // predicted_qs
      acc[2] += a.info_w * sc[2] * a.inv_batch;  // target_qs
    }
    if (a.info_mode & 2) {  // actor + temperature step (sac.py:193-234)
      const float alpha = a.alpha[0];
      acc[3] = -(sc[3] - alpha * sc[4]) * a.inv_batch;  // actor_loss
      acc[4] = alpha;                                   // temperature
      acc[5] = -sc[4] * a.inv_batch;                    // entropy
      acc[6] = alpha * (-sc[5] * a.inv_batch - a.target_entropy);  // temperature_loss
    }
  }
  // clip_by_global_norm (optimizers.py:36-37): g <- g * max_norm / ||g|| when ||g|| >= max_norm
  float cs_c = 1.f, cs_a = 1.f;
  if (a.clip_c > 0.f && a.critic_on) { const float n = sqrtf(a.norm2[0]); if (!(n < a.clip_c)) cs_c = a.clip_c / n; }
  if (a.clip_a > 0.f && a.actor_on) { const float n = sqrtf(a.norm2[1]); if (!(n < a.clip_a)) cs_a = a.clip_a / n; }
  const long i4 = 4 * t;
  const bool c_all = i4 + 3 < a.Pc, c_none = i4 >= a.Pc;
  const bool a_all = i4 >= a.Pa0 && i4 + 3 < a.Pa1, a_none = i4 + 3 < a.Pa0 || i4 >= a.Pa1;
  if (a.vec_ok && i4 + 3 < a.P - 1 && (c_all || c_none) && (a_all || a_none)) {
    const float b1 = 0.9f, b2 = 0.999f, eps = 1e-8f;
    const long ic = c_all ? i4 : 0, ka = a_all ? i4 - a.Pa0 : 0;
    const float4 p0 = *reinterpret_cast<const float4*>(a.theta + i4);
    const float4 tt = *reinterpret_cast<const float4*>((a.ema_on ? a.theta_target : a.theta) + i4);
    const float4 gc = *reinterpret_cast<const float4*>(a.g_critic + ic);
    const float4 mc = *reinterpret_cast<const float4*>(a.m_c + ic), vc = *reinterpret_cast<const float4*>(a.v_c + ic);
    // (the actor support starts at an arbitrary leaf offset -- behind the critic head's 1-element bias: its arrays are indexed by
    //  i - Pa0 and only 4-byte aligned; global 16-byte accesses need no more)
    const f32x4 ga = *reinterpret_cast<const f32x4u*>(a.g_actor + ka);
    const f32x4 ma = *reinterpret_cast<const f32x4u*>(a.m_a + ka), va = *reinterpret_cast<const f32x4u*>(a.v_a + ka);
    const float p0e[4] = {p0.x, p0.y, p0.z, p0.w}, tte[4] = {tt.x, tt.y, tt.z, tt.w};
    const float gce[4] = {gc.x, gc.y, gc.z, gc.w}, mce[4] = {mc.x, mc.y, mc.z, mc.w}, vce[4] = {vc.x, vc.y, vc.z, vc.w};
    const float gae[4] = {ga[0], ga[1], ga[2], ga[3]}, mae[4] = {ma[0], ma[1], ma[2], ma[3]}, vae[4] = {va[0], va[1], va[2], va[3]};
    float pn[4], tn[4], mcn[4], vcn[4], man[4], van[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float ua = 0.f, uc = 0.f;
      {
        const float g = a.critic_on ? gce[e] * cs_c : 0.f;
        const float m = b1 * mce[e] + (1.f - b1) * g;
        const float v = b2 * vce[e] + (1.f - b2) * g * g;
        mcn[e] = m; vcn[e] = v;
        if (c_all) uc = -a.lr_c * (m / a.bc1) / (sqrtf(v / a.bc2) + eps);
      }
      {
        const float g = a.actor_on ? gae[e] * cs_a : 0.f;
        const float m = b1 * mae[e] + (1.f - b1) * g;
        const float v = b2 * vae[e] + (1.f - b2) * g * g;
        man[e] = m; van[e] = v;
        if (a_all) ua = -a.lr_a * (m / a.bc1) / (sqrtf(v / a.bc2) + eps);
      }
      float ut = 0.f;
      if (a.wd_a != 0.f) ua -= a.lr_a * a.wd_a * p0e[e];
      if (a.wd_c != 0.f) uc -= a.lr_c * a.wd_c * p0e[e];
      if (a.wd_t != 0.f) ut -= a.lr_t * a.wd_t * p0e[e];
      pn[e] = p0e[e] + ((ua + uc) + ut);
      tn[e] = pn[e] * a.tau + tte[e] * (1.f - a.tau);
    }
    if (c_all) {
      *reinterpret_cast<float4*>(a.m_c + i4) = make_float4(mcn[0], mcn[1], mcn[2], mcn[3]);
      *reinterpret_cast<float4*>(a.v_c + i4) = make_float4(vcn[0], vcn[1], vcn[2], vcn[3]);
    }
    if (a_all) {
      *reinterpret_cast<f32x4u*>(a.m_a + ka) = (f32x4){man[0], man[1], man[2], man[3]};
      *reinterpret_cast<f32x4u*>(a.v_a + ka) = (f32x4){van[0], van[1], van[2], van[3]};
    }
    *reinterpret_cast<float4*>(a.theta + i4) = make_float4(pn[0], pn[1], pn[2], pn[3]);
    if (a.ema_on) *reinterpret_cast<float4*>(a.theta_target + i4) = make_float4(tn[0], tn[1], tn[2], tn[3]);
    return;
  }
  const long total = a.P + a.n_frozen_live;
#pragma unroll 1
  for (int e = 0; e < 4; ++e)
    if (i4 + e < total) adam_elem(a, i4 + e, cs_c, cs_a);
}

// `steps` deferred target-EMA steps of the frozen trunk leaves at once (common.py:124-134 on leaves no gradient or weight decay
// ever touches): t <- p*tau + t*(1-tau), repeated -- the same expression, hence the same rounding sequence, as adam_ema_kernel
// applies step by step.  The iteration stops at its fixed point (t no longer changes), which a constant p reaches after a few steps.
__global__ __launch_bounds__(256) void frozen_ema_kernel(const float* frozen, float* frozen_target, long n, float tau, long steps) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float p = frozen[i];
  float t = frozen_target[i];
  for (long k = 0; k < steps; ++k) {
    const float u = p * tau + t * (1.f - tau);
    if (u == t) break;
    t = u;
  }
  frozen_target[i] = t;
}
int frozen_ema(const float* frozen, float* frozen_target, long n, float tau, long steps, hipStream_t stream) {
  if (n <= 0 || steps <= 0) return SERL_OK;
  SERL_LAUNCH_CHAIN(frozen_ema_kernel, dim3(cdiv(n, 256)), dim3(256), 0, stream, frozen, frozen_target, n, tau, steps);
  SERL_HIP(hipGetLastError());
  return SERL_OK;
}

int adam_ema(const AdamArgs& a, hipStream_t stream) {
  ProfScope prof("adam_ema", stream);
  const bool frozen = a.n_frozen > 0 && (a.ema_on || a.wd_c != 0.f || a.wd_a != 0.f || a.wd_t != 0.f);
  AdamArgs v = a;
  v.n_frozen_live = frozen ? a.n_frozen : 0;
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  v.vec_ok = a.Pc >= 4 && a.Pa1 - a.Pa0 >= 4 && al16(a.theta) && al16(a.theta_target) && al16(a.g_critic) && al16(a.m_c) &&
             al16(a.v_c) && a.g_critic && a.g_actor && a.m_a && a.v_a;
  SERL_LAUNCH_CHAIN(adam_ema_kernel, dim3(cdiv(cdiv(a.P + v.n_frozen_live, 4), 256)), dim3(256), 0, stream, v);
  SERL_HIP(hipGetLastError());
  return SERL_OK;
}

// The info rider of adam_ema_kernel alone: one workgroup of that kernel over an EMPTY index space (P = 0, no frozen leaves), so
// thread 0 forms the info scalars with the instructions an update forms them with -- the same bits -- and no thread reaches a
// parameter, a moment or a target (serl_agent_eval_losses).
int adam_info_only(const AdamArgs& a, hipStream_t stream) {
  AdamArgs v = a;
  v.P = v.Pc = v.Pa0 = v.Pa1 = 0;
  v.n_frozen = v.n_frozen_live = 0;
  v.vec_ok = 0;
  v.critic_on = v.actor_on = v.temp_on = v.ema_on = 0;
  v.clip_c = v.clip_a = v.clip_t = 0.f;
  SERL_REQUIRE(v.info_mode != 0 && v.info_acc && v.scalars, "the info rider needs its mode, its scalars and a place for the result");
  SERL_LAUNCH_CHAIN(adam_ema_kernel, dim3(1), dim3(256), 0, stream, v);
  SERL_HIP(hipGetLastError());
  return SERL_OK;
}

// squared global norms of the two gradient ranges (clip_by_global_norm): one 1024-thread block per range, fp64 partials
__global__ __launch_bounds__(1024) void grad_norm2_kernel(const float* gc, long nc, const float* ga, long na, float* out) {
  const float* g = blockIdx.x ? ga : gc;
  const long n = blockIdx.x ? na : nc;
  double s = 0.0;
  for (long i = threadIdx.x; i < n; i += 1024) s += (double)g[i] * (double)g[i];
  __shared__ double red[1024];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = (float)red[0];
}
int grad_norm2(const float* g_critic, long nc, const float* g_actor, long na, float* out, hipStream_t stream) {
  SERL_LAUNCH_CHAIN(grad_norm2_kernel, dim3(2), dim3(1024), 0, stream, g_critic, nc, g_actor, na, out);
  SERL_HIP(hipGetLastError());
  return SERL_OK;
}

// =============================================================================================
// device noise (production mode): counter-based hash -> N(0,1) and Bernoulli(keep) masks
// =============================================================================================
__device__ __forceinline__ void gen_one(const NoiseJob& j, long i0) {
  if (i0 >= j.n) return;
  long i = i0;  // position in the global tensor
  if (j.rows_global) {
    const long e = i0 % j.row_elems, rr = i0 / j.row_elems, r = rr % j.rows_local, plane = rr / j.rows_local;
    i = (plane * j.rows_global + j.row_offset + r) * j.row_elems + e;
  }
  if (j.kind == 0) {
    const uint64_t r = mix64(j.seed ^ mix64((uint64_t)i));
    const float u1 = ((float)(uint32_t)(r >> 40) + 1.0f) * (1.0f / 16777217.0f);
    const float u2 = (float)(uint32_t)((r >> 8) & 0xFFFFFF) * (1.0f / 16777216.0f);
    static_cast<float*>(j.out)[i0] = sqrtf(-2.f * logf(u1)) * cosf(6.283185307179586f * u2);
  } else {
    const uint64_t r = mix64(j.seed ^ mix64((uint64_t)i + 0x51ED270Bull));
    static_cast<uint8_t*>(j.out)[i0] = ((float)(uint32_t)(r >> 40) * (1.0f / 16777216.0f)) < j.keep ? 1 : 0;
  }
}
// all the noise of one update phase in one launch: blockIdx.y = job (a normal tensor or a keep-mask)
__global__ void gen_noise_kernel(Multi<NoiseJob> mv) {
  gen_one(mv.v[blockIdx.y], (long)blockIdx.x * 256 + threadIdx.x);
}
int gen_noise_multi(const NoiseJob* vs, int n, hipStream_t stream) {
  SERL_REQUIRE(n >= 1 && n <= kMaxMulti, "bad job count %d", n);
  Multi<NoiseJob> mv{};
  long nmax = 0;
  for (int i = 0; i < n; ++i) { mv.v[i] = vs[i]; nmax = std::max(nmax, vs[i].n); }
  SERL_LAUNCH_CHAIN(gen_noise_kernel, dim3(cdiv(nmax, 256), n), dim3(256), 0, stream, mv);
  SERL_HIP(hipGetLastError());
  return SERL_OK;
}
}  // namespace serl
