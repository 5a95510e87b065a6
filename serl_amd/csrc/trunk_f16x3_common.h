// Part of the split-fp16 trunk (trunk_f16x3.hip includes these in order; round 6 split the 2,600-line file by kernel family):
// shared by every split-fp16 trunk kernel: argument structs, the hi / lo' split, LDS swizzle, the tile tickets and the
// statistics exchange of the fused GroupNorm epilogues, the C-layout fused store (register-staged and LDS-DMA kernels).
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "gn_exchange.h"
#include "prof.h"
#include "trunk_common.h"

namespace serl {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
constexpr float kLoScale = 2048.0f, kLoInv = 1.0f / 2048.0f;  // 2^11

// GroupNorm (+ residual) + ReLU + split8 re-layout in the PRODUCING conv's epilogue (mode != 0) instead of a separate
// elementwise pass over the raw fp32 tensor.  GroupNorm needs the statistics of the whole image.  Where a tile IS a whole image
// over complete groups (or a wave's block is: LOCAL, expected == 0) they are taken inside the workgroup and nothing leaves it.
// Otherwise G = 2..8 workgroups produce them: each PUBLISHES its partial sums as one record of data-tagged granules and reads the
// records of the image's other tiles until every granule carries this pass's tag (gnx_publish / gnx_collect below, gn_exchange.h).
// FORWARD PROGRESS.  Tiles are handed out by atomic TICKETS taken when a workgroup starts running (fused_tile): one
// counter per XCD, each covering a contiguous range of whole images, so the G tiles of an image carry CONSECUTIVE tickets
// of one counter (and are fetched through one L2).  A waiting workgroup therefore waits (a) for tiles that running
// workgroups already hold -- they finish without waiting for anybody -- or (b) for not-yet-taken tiles of the ONE image
// per counter that straddles its next ticket; at most G - 1 workgroups per counter can wait in state (b), so as long as
// more than 8 (G - 1) workgroups are resident, one of them is running or about to start and takes the missing tickets
// (a workgroup whose own XCD's range is used up takes from the next XCD's counter).  The pass plan checks that bound
// against the CUs the stream may use (resident_workgroups) and falls back to the separate elementwise pass otherwise;
// the spin itself is bounded (trap) so a protocol error aborts the kernel instead of hanging the GPU.
// Wave priority of the trunk's conv kernels (s_setprio 3).  In the pipelined step the frozen trunk's stream IS the critical path and the
// update chain's workgroups share its SIMDs (they are sized to fit beside two trunk workgroups per CU): the arbiter then prefers the
// trunk's waves.  Same-call A/B (profiles/r05_ab_wave_prio.txt): pipelined 2.4176 / 2.4124 -> 2.4004 / 2.3992 ms (stage-0 convs
// -13 .. -22 us, conv_init -20 us; the chain's kernels move under the later convs, +6 .. +10 us there), serial unchanged, one rank of
// eight (128 images per pass, where the CHAIN is the critical path) 0.6788 -> 0.6862: on from 512 images per pass.  Value 2 (the default
// when on): 3 in the main loop, 1 in the block convs' epilogues -- an epilogue (HBM traffic, conversions, the wait for the image's other
// tiles) then yields the SIMD to the main loop of the CU's other workgroup: 2.391 / 2.4062 (flat 3) -> 2.3824 / 2.3987, same call.
// (SERL_TRUNK_WPRIO, the switch that forced off / flat / main-loop-over-epilogue, went with round 6: the policy is fixed.)
static int trunk_wave_prio(long images) { return images >= 512 ? 2 : 0; }

struct FuseArgs {
  int mode;                 // 0 off; 1 relu(GN(y)); 2 relu(GN(y) + res_split); 3 relu(GN(y) + GN_res(res_raw))
  int expected;             // row tiles per image = records a tile's statistics are summed from; 0 = LOCAL: the statistics of an
                            // (image, group) lie inside one workgroup (a whole-image row-slab tile; a wave's 64 x 64 block in stage 2;
                            // eight whole images per tile in stage 3) -- no ticket, no record, no wait
  uint64_t* rec;            // this layer's records [tile][kGnxGranules] (gn_exchange.h); written and read with system-scope accesses only
  uint32_t epoch;           // tag of this pass's granules, never 0
  int* ticket;              // [8] per-XCD tile counters, zeroed per pass
  int group;                // G: tiles (workgroups) per image -- tickets of one image are consecutive
  GnRef gn;                 // this conv's scale, bias and 1 / count (a fused launch writes no statistics: nothing reads them)
  GnRef res_gn;             // mode 3: the projection's GroupNorm (complete: that conv ran before)
  const uint8_t* res_split; // mode 2: the block input (split8)
  const float* res_raw;     // mode 3: raw projection output
  uint8_t* out_split;       // split8 output
  float* out_f32;           // instead of out_split when set: plain fp32 NHWC output (the last block's conv1 writes the trunk's features)
};

struct ConvArgsB {
  ConvArgs c;           // .w unused
  FuseArgs fz;
  const uint16_t* whi;  // [Cout][K]
  const uint16_t* wlo;
  const float* winv;    // [Cout] 1 / (per-output-channel weight scale)
  const uint16_t* wdma;  // LDS-DMA kernel: the planes in its piece order (pack_dma_order_f16x3) or nullptr
  int K;
  // row-slab kernel, fused epilogue: the SECOND workgroup of every CU (block ids 256..511 of the first round) starts
  // `stagger` x s_sleep(127) late (before it takes its tile ticket), see the kernel
  int stagger;
  int wprio;   // wave priority (s_setprio) of the kernel's waves: the frozen trunk is the step's critical path, the chain's waves that share a SIMD are not
};

// LDS-DMA kernel, default since round 5 (SERL_PROJ_FUSE=0 switches it off): the block's 1x1 stride-2 projection computed by the SAME workgroup in front of its
// 3x3 stride-2 conv0 tile (same input, same output tile: the projection's pixel is conv0's tap (0, 0)).  A separate kernel
// parameter behind the existing ones, and a separate instantiation (PROJ): the kernels without it keep their code and their
// argument offsets.
struct ConvProjB {
  const uint16_t* wdma;  // the projection's planes in piece order (K = Cin)
  const float* winv;     // [Cout]
  float* out;            // raw fp32 [M][Cout]
  double* stats;         // [N][4][2]
};

typedef __fp16 h16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float clamp_h(float v) { return __builtin_amdgcn_fmed3f(v, -65504.0f, 65504.0f); }

// float4 -> 4 fp16 hi (packed in uint2) and 4 fp16 lo' = fp16((x - hi) * 2^11).
// hi is converted with v_cvt_pkrtz (any hi within one fp16 ulp works: the residual is exact in fp32 and
// stays in range after the 2^11 scale); lo' is rounded to nearest (v_cvt_pk_f16_f32), so
// |x - hi - 2^-11 lo'| <= 2^-21 |x|.  Activations are GroupNorm outputs (|x| << 65504): no clamp here,
// the one-time weight packing clamps.
__device__ __forceinline__ void split4(const float4 v, uint2& hi, uint2& lo) {
  const h16x2 h0 = __builtin_amdgcn_cvt_pkrtz(v.x, v.y);
  const h16x2 h1 = __builtin_amdgcn_cvt_pkrtz(v.z, v.w);
  const f32x2 r0 = {(v.x - (float)h0[0]) * kLoScale, (v.y - (float)h0[1]) * kLoScale};
  const f32x2 r1 = {(v.z - (float)h1[0]) * kLoScale, (v.w - (float)h1[1]) * kLoScale};
  const f16x2 l0 = __builtin_convertvector(r0, f16x2), l1 = __builtin_convertvector(r1, f16x2);
  hi = make_uint2(__builtin_bit_cast(unsigned, h0), __builtin_bit_cast(unsigned, h1));
  lo = make_uint2(__builtin_bit_cast(unsigned, l0), __builtin_bit_cast(unsigned, l1));
}

// byte offset of 16-byte slot `slot` (0..3) of row `row` in a [rows][32] bf16 plane (64-byte rows)
__device__ __forceinline__ int swz(int row, int slot) { return row * 64 + ((slot ^ ((row >> 2) & 3)) << 4); }

// Tile of this workgroup in a fused launch of `ntiles` = gridDim.x tiles, `group` tiles per image.  The images are
// split into 8 contiguous ranges (one per XCD, as xcd_remap does for block ids); a workgroup draws from the counter of the
// XCD it actually runs on (HW_REG_XCC_ID -- used for L2 affinity only, any value 0..7 is correct) and moves on to the next
// XCD's counter when that range is used up.  #workgroups == #tiles and every valid ticket is unique, so every workgroup
// finds a tile within one round over the 8 counters.
__device__ __forceinline__ int fused_tile(const FuseArgs& fz, int ntiles) {
  __shared__ int s_tile;
  if (threadIdx.x == 0) {
    const int G = fz.group, ngroups = ntiles / G, gq = ngroups >> 3, gr = ngroups & 7;
    unsigned x;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
    x &= 7u;
    int tile = -1;
    for (int k = 0; k < 8 && tile < 0; ++k, x = (x + 1) & 7u) {
      const int g0 = (int)x < gr ? (int)x * (gq + 1) : gr * (gq + 1) + ((int)x - gr) * gq;
      const int cnt = (gq + ((int)x < gr ? 1 : 0)) * G;
      if (cnt == 0) continue;
      const int t = __hip_atomic_fetch_add(fz.ticket + x, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      if (t < cnt) tile = g0 * G + t;
    }
    if (tile < 0) __builtin_trap();   // cannot happen: as many workgroups as tiles
    s_tile = tile;
  }
  __syncthreads();
  return s_tile;
}

// THE EXCHANGE.  What a tile hands to the other tiles of its image is 16 or 32 fp32 partial sums.  Each travels as a GRANULE: one
// naturally aligned 8-byte {value, tag} written by ONE system-scope store (global_store_dwordx2 sc0 sc1: write-through, past the 8
// per-XCD L2s -- an image's workgroups can sit on different XCDs) and read by system-scope loads (global_load_dwordx2 sc0 sc1:
// never served from a CU's L1).  The data is its own flag: a reader that sees this pass's tag in a granule has, from the same
// load, the value that was stored with it, so the protocol needs NO ordering between memory operations -- no returning atomics,
// no drain before a flag, no arrival counter, no separate statistics loads: a tile publishes and does not wait for its store,
// and the last arriver's peers are complete one load round trip after its store lands.  That an aligned 8-byte store is never
// observed torn is MEASURED gfx950 behaviour (ROCm 7.2), not an architectural guarantee; the reproducibility test of
// tests/test_gn_exchange_gpu.py (bit-identical passes under uneven load) is what a torn or stale granule would break.
// Tags are the workspace's pass epoch (gn_exchange.h: never 0, records zeroed before the first pass and at the wrap), every tile
// has a record of its own per layer, so nothing is zeroed between passes and nothing is reused within one.
// The statistics are what they were -- the fp64 sum of the same per-wave fp32 partials -- but in a FIXED order (a granule's
// values over the image's tiles in tile order, then the waves, then a group's segments in channel order), where the fp64
// atomics they replace added in arrival order: every pass over the same frames now gives the same bits.
//
// LAYOUT 0: row-slab tile, four waves over the SAME 64 channels, s_part[wave][segment * 2 + stat] (4 segments of 16 channels);
// LAYOUT TN = 1 / 2: LDS-DMA tile, wave = wm * 2 + wn over columns wn * 32 TN .., s_part[wave][(tn * 2 + segment) * 2 + stat].
template <int LAYOUT>
struct GnxShape {
  static constexpr int NP = LAYOUT == 0 ? 8 : 4 * LAYOUT;    // partials per wave
  static constexpr int NG = 4 * NP;                          // granules of a record in use
  static constexpr int NSEG = LAYOUT == 0 ? 4 : 4 * LAYOUT;  // 16-channel segments of the tile
  static constexpr int NC = LAYOUT == 0 ? 4 : 2;             // waves that hold rows of one segment
  static_assert(NG <= kGnxGranules, "a record holds the tile's partials");
  // granule of the c-th contributing wave of tile segment `seg`
  __device__ static __forceinline__ int granule(int c, int seg, int stat) {
    if (LAYOUT == 0) return c * NP + seg * 2 + stat;
    const int per_wave = 2 * LAYOUT, wn = seg / per_wave, j = seg - wn * per_wave;
    return (c * 2 + wn) * NP + j * 2 + stat;
  }
};
typedef __attribute__((address_space(1))) unsigned long long gnx_u64;

// gnx_publish + gnx_collect are called by every thread of the workgroup BEHIND the barrier that completed s_part (the tile's NG
// partials, wave-major); only wave 0 touches memory in them.  Publish: wave 0 stores the record of tile `tile` and does not wait
// for it.  Collect (as late as the caller has other work to issue): wave 0 polls the image's other records and leaves mean / rstd
// of every 16-channel segment of the tile (channels n0 + 16 seg ..) in s_mr; the closing barrier hands them to all waves.
// The spin is bounded (trap): a protocol error aborts the kernel instead of hanging the GPU; a real wait is a few microseconds.
template <int LAYOUT>
__device__ __forceinline__ void gnx_publish(const FuseArgs& fz, int tile, int wave, int lane, const float* s_part) {
  using S = GnxShape<LAYOUT>;
  if (wave == 0 && lane < S::NG)
    __hip_atomic_store((gnx_u64*)fz.rec + (size_t)tile * kGnxGranules + lane,
                       (unsigned long long)gnx_pack(__builtin_bit_cast(uint32_t, s_part[lane]), fz.epoch), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
}
template <int LAYOUT>
__device__ __forceinline__ void gnx_collect(const FuseArgs& fz, int tile, int tiles_n, int n0, int wave, int lane, const float* s_part,
                                            float (*s_mr)[2]) {
  using S = GnxShape<LAYOUT>;
  __shared__ double s_acc[S::NG];
  if (wave == 0) {
    gnx_u64* const rec = (gnx_u64*)fz.rec;
    const GnxPeers pr = gnx_peers(tile, fz.expected, tiles_n);
    const int gl = lane & (S::NG - 1);   // (lanes past NG repeat granules: same lines, no extra traffic, no divergence)
    const float mine = s_part[gl];
    double acc;
    for (int spins = 0;; ++spins) {
      bool ok = true;
      acc = 0.0;
      for (int p0 = 0; p0 < pr.count; p0 += 4) {   // four records' loads in flight together
        unsigned long long x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          x[k] = gnx_pack(__builtin_bit_cast(uint32_t, mine), fz.epoch);   // (its own partials come from LDS, not from memory)
          if (p0 + k < pr.count && p0 + k != pr.self)
            x[k] = __hip_atomic_load(rec + (size_t)(pr.first + (long)(p0 + k) * pr.stride) * kGnxGranules + gl, __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_SYSTEM);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (p0 + k < pr.count) {
            ok = ok && gnx_tag(x[k]) == fz.epoch;
            acc += (double)__builtin_bit_cast(float, gnx_value(x[k]));
          }
      }
      if (__all(ok)) break;
      __builtin_amdgcn_s_sleep(4);
      if (spins > (1 << 22)) __builtin_trap();
    }
    if (lane < S::NG) s_acc[gl] = acc;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   // (this wave's LDS writes before its own reads below)
    __builtin_amdgcn_wave_barrier();
    if (lane < S::NSEG) {
      const int gsize = fz.gn.gsize, g = (n0 + 16 * lane) / gsize;
      double s = 0.0, q = 0.0;
      for (int seg = 0; seg < S::NSEG; ++seg)
        if ((n0 + 16 * seg) / gsize == g)
          for (int c = 0; c < S::NC; ++c) { s += s_acc[S::granule(c, seg, 0)]; q += s_acc[S::granule(c, seg, 1)]; }
      const double mean = s * fz.gn.inv_count, m2 = q * fz.gn.inv_count;
      const float var = fmaxf((float)(m2 - mean * mean), 0.f);
      s_mr[lane][0] = (float)mean;
      s_mr[lane][1] = rsqrtf(var + 1e-5f);
    }
  }
  __syncthreads();
}

// GroupNorm scale / shift of one channel from the COMPLETE statistics of an earlier launch
__device__ __forceinline__ void gn_coef1(const GnRef& g, int n, int c, float& sc, float& sh) {
  const double* st = g.stats + ((size_t)n * kGnGroups + c / g.gsize) * 2;
  const double mean = st[0] * g.inv_count, m2 = st[1] * g.inv_count;
  const float var = fmaxf((float)(m2 - mean * mean), 0.f);
  const float rstd = rsqrtf(var + 1e-5f), mf = (float)mean;
  sc = g.gamma[c] * rstd;
  sh = g.beta[c] - mf * sc;
}

__device__ __forceinline__ uint32_t swap_adjacent_lanes(uint32_t v) {   // quad_perm [1, 0, 3, 2]
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);
}
__device__ __forceinline__ float half_bits_to_float(uint32_t b) {
  return (float)__builtin_bit_cast(_Float16, (uint16_t)(b & 0xffffu));
}

// The MFMA C layout gives a lane ONE channel (col0 + 32 tn + li) of 16 rows per 32x32 tile; the split8 layout wants
// the 8 hi halves of 8 consecutive channels in one 16-byte unit and their lo' halves in the next.  Adjacent lanes
// (channels c, c+1) trade halves: the even lane ends up with the dword of the two hi halves, the odd lane with the dword
// of the two lo' halves, so 32 lanes write the same contiguous 128 bytes a row of 32 fp32 values took.  Two rows are
// processed together (packed fp32 math, one cvt_pkrtz / cvt_pk per pair, ONE lane exchange per pair): the epilogue's
// VALU work competes with the other workgroup's MFMAs on the same SIMD, so instruction count matters here.
template <int TM, int TN>
struct FusedResidual { uint32_t v[TM][TN][16]; };

// residual operand of this lane's elements, loaded BEFORE the statistics wait so the latency hides behind it
template <int TM, int TN>
__device__ __forceinline__ void fused_load_residual(const ConvArgsB& ab, FusedResidual<TM, TN>& res, int wrow0, int col0,
                                                    int li, int lh) {
  const FuseArgs& fz = ab.fz;
  if (fz.mode < 2) return;
  const int Cout = ab.c.Cout;
  const bool odd = li & 1;
#pragma unroll
  for (int tm = 0; tm < TM; ++tm)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = wrow0 + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
      const size_t rowb = (size_t)m * Cout * 4;
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) {
        const int c = col0 + tn * 32 + li;
        if (fz.mode == 2) res.v[tm][tn][r] = *reinterpret_cast<const uint32_t*>(fz.res_split + rowb + (c & ~7) * 4 + (odd ? 16 : 0) + (c & 6) * 2);
        else res.v[tm][tn][r] = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(fz.res_raw) + rowb + c * 4);
      }
    }
}

// The statistics come from the caller (taken inside the workgroup, LOCAL, or out of gnx_collect): mean[] / rstd[] hold one value per
// slot, and with PER_TN one per (32-column block tn, slot) at [tn * NSLOT + slot] -- a wave's 64 columns span two 32-channel groups.
// NSLOT = 4 (stage 3, images of 16 pixels): the wave's 64 rows are FOUR images, slot s = rows 16 s .. 16 s + 15 = image n_img + s, each with
// its own statistics; NSLOT = 1: the whole block lies in image n_img.
template <int TM, int TN, int NSLOT = 1, bool PER_TN = false>
__device__ __forceinline__ void fused_gn_store(const ConvArgsB& ab, const f32x16 (&acc)[TM][TN],
                                               const FusedResidual<TM, TN>& res, int n_img, int wrow0, int col0, int li, int lh,
                                               const float* mean, const float* rstd) {
  const FuseArgs& fz = ab.fz;
  const int Cout = ab.c.Cout;
  const bool odd = li & 1;
  // v_perm selectors (byte k of the result: 0..3 = bytes of the 2nd operand, 4..7 = bytes of the 1st)
  const uint32_t sel_r0 = odd ? 0x01000504u : 0x05040100u;   // (keep, recv) low halves  -> even: keep|recv<<16, odd: recv|keep<<16
  const uint32_t sel_r1 = odd ? 0x03020706u : 0x07060302u;   // same for the high halves
  const uint32_t sel_lo = 0x05040100u, sel_hi = 0x07060302u; // (a.lo16 | b.lo16 << 16), (a.hi16 | b.hi16 << 16) of perm(b, a, .)
#pragma unroll
  for (int tn = 0; tn < TN; ++tn) {
    const int c = col0 + tn * 32 + li;
    float scs[NSLOT], shs[NSLOT], rss[NSLOT], rhs[NSLOT];
#pragma unroll
    for (int sl = 0; sl < NSLOT; ++sl) {
      rss[sl] = 0.f; rhs[sl] = 0.f;
      const int si = (PER_TN ? tn * NSLOT : 0) + sl;
      scs[sl] = fz.gn.gamma[c] * rstd[si];
      shs[sl] = fz.gn.beta[c] - mean[si] * scs[sl];
      if (fz.mode >= 3) gn_coef1(fz.res_gn, n_img + sl, c, rss[sl], rhs[sl]);
    }
    const int cbyte = (c & ~7) * 4 + (odd ? 16 : 0) + (c & 6) * 2;
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
      for (int rp = 0; rp < 8; ++rp) {
        const int r0 = 2 * rp, r1 = r0 + 1;   // rows m and m + 1 (same 16-row slot)
        const int sl = NSLOT == 1 ? 0 : 2 * tm + (r0 >> 3);
        const f32x2 sc2 = {scs[sl], scs[sl]}, sh2 = {shs[sl], shs[sl]}, rs2 = {rss[sl], rss[sl]}, rh2 = {rhs[sl], rhs[sl]};
        const int m = wrow0 + tm * 32 + (r0 & 3) + 8 * (r0 >> 2) + 4 * lh;
        f32x2 v = (f32x2){acc[tm][tn][r0], acc[tm][tn][r1]} * sc2 + sh2;
        if (fz.mode == 2) {
          const uint32_t o0 = res.v[tm][tn][r0], o1 = res.v[tm][tn][r1];
          // what the neighbour needs from me (even: my hi16 = hi[c+1]; odd: my lo16 = lo[c-1]) and what I keep
          const uint32_t send = __builtin_amdgcn_perm(o1, o0, odd ? sel_lo : sel_hi);
          const uint32_t mine = __builtin_amdgcn_perm(o1, o0, odd ? sel_hi : sel_lo);
          const uint32_t recv = swap_adjacent_lanes(send);
          const uint32_t H = odd ? recv : mine, L = odd ? mine : recv;   // (x_hi row0 | x_hi row1 << 16), same for lo'
          const f16x2 Hh = __builtin_bit_cast(f16x2, H), Lh = __builtin_bit_cast(f16x2, L);
          const f32x2 xh = {(float)Hh[0], (float)Hh[1]}, xl = {(float)Lh[0], (float)Lh[1]};
          v = (xh + xl * (f32x2){kLoInv, kLoInv}) + v;
        } else if (fz.mode == 3) {
          const f32x2 x = {__builtin_bit_cast(float, res.v[tm][tn][r0]), __builtin_bit_cast(float, res.v[tm][tn][r1])};
          v = (x * rs2 + rh2) + v;
        } else if (fz.mode == 4) {   // residual = relu(GroupNorm(raw)): the block input that was never materialised (RAWIN)
          const f32x2 x = {__builtin_bit_cast(float, res.v[tm][tn][r0]), __builtin_bit_cast(float, res.v[tm][tn][r1])};
          const f32x2 y = x * rs2 + rh2;
          v = (f32x2){fmaxf(y[0], 0.f), fmaxf(y[1], 0.f)} + v;
        }
        v = (f32x2){fmaxf(v[0], 0.f), fmaxf(v[1], 0.f)};
        if (fz.out_f32) {   // (uniform) plain fp32 output: the trunk's features
          float* o32 = fz.out_f32 + (size_t)m * Cout + c;
          o32[0] = v[0];
          o32[Cout] = v[1];
          continue;
        }
        const h16x2 hp = __builtin_amdgcn_cvt_pkrtz(v[0], v[1]);
        const f32x2 hf = {(float)hp[0], (float)hp[1]};
        const f16x2 lp = __builtin_convertvector((v - hf) * (f32x2){kLoScale, kLoScale}, f16x2);
        const uint32_t hpb = __builtin_bit_cast(uint32_t, hp), lpb = __builtin_bit_cast(uint32_t, lp);
        const uint32_t keep = odd ? lpb : hpb;
        const uint32_t recv = swap_adjacent_lanes(odd ? hpb : lpb);
        uint8_t* o = fz.out_split + (size_t)m * Cout * 4 + cbyte;
        *reinterpret_cast<uint32_t*>(o) = __builtin_amdgcn_perm(recv, keep, sel_r0);
        *reinterpret_cast<uint32_t*>(o + (size_t)Cout * 4) = __builtin_amdgcn_perm(recv, keep, sel_r1);
      }
  }
}

}  // namespace serl
