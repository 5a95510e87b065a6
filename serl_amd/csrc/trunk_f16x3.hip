// Split-fp16 ("f16x3") implicit-GEMM conv for the frozen ResNet-10 trunk on MI355X (gfx950).
//
// fp32 operands are split on the fly into  x = hi + 2^-11 * lo'  with hi = fp16(x) and
// lo' = fp16((x - hi) * 2^11)  (the residual is exact in fp32 and the 2^11 scale keeps it in fp16's
// normal range), and every fp32 product is replaced by three fp16 MFMA products accumulated in fp32:
//     a*b ~= a_hi*b_hi + 2^-11 * (a_hi*b_lo' + a_lo'*b_hi)       (the 2^-22 a_lo'*b_lo' term is dropped)
// on v_mfma_f32_32x32x16_f16, whose dense rate is 16x the f32-input MFMA: 3 instructions of 32 cycles
// per 32x32x16 block instead of 8 of 64.  The hi*hi products and the cross products go to separate
// fp32 accumulators that are combined once in the epilogue.  Per-product relative error <= ~3*2^-22
// (7e-7), i.e. fp32-roundoff class; measured error of the whole trunk vs fp64 in tests/test_agent_gpu.py
// next to the exact-fp32 kernel's (every parity test runs in both modes).
//
// Same structure as conv_igemm_kernel (trunk.hip): NHWC activations stay fp32 in HBM, BK = 32 chunks
// inside one (ky,kx) tap, GroupNorm+ReLU of the producer applied on load, GN statistics in the
// epilogue.  Differences: weights are pre-split and pre-transposed once to fp16 [Cout][K] (hi, lo');
// LDS holds fp16 hi/lo' planes with K contiguous (64-byte rows, 16-byte slots XOR-swizzled by
// (row>>2)&3 -> conflict-free ds_read_b128 MFMA fragments).
//
// The kernels live in headers by family (round 6): trunk_f16x3_common.h (structs, split, fused-epilogue exchange), _igemm.h
// (register-staged implicit GEMM), _dma.h (LDS-DMA ring kernel), _rowslab.h (row-slab kernels), _conv_init.h (u8 conv_init + pool),
// _elementwise.h (statistics, weight packing, split8 producers); this file keeps the kernel selection and the pass itself.
#include "trunk_f16x3_elementwise.h"

namespace serl {

// Workgroups of a 2-per-CU conv kernel that can be co-resident on `stream`, counted conservatively as ONE per compute unit
// the stream may use (its CU mask if it has one; a CPX-partitioned device reports 32 CUs).  Cached per stream.
static int resident_workgroups(hipStream_t stream) {
  thread_local hipStream_t last = nullptr;
  thread_local int last_n = -1;
  if (last_n >= 0 && last == stream) return last_n;
  int dev = 0, n = 0;
  hipDeviceProp_t prop;
  if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) n = prop.multiProcessorCount;
  uint32_t mask[16] = {0};
  if (hipExtStreamGetCUMask(stream, 16, mask) == hipSuccess) {
    int m = 0;
    for (uint32_t w : mask) m += __builtin_popcount(w);
    if (m > 0 && (n == 0 || m < n)) n = m;
  } else {
    (void)hipGetLastError();
  }
  last = stream; last_n = n;
  return n;
}

// Geometry of conv k (0 conv0, 1 conv1, 2 projection) of residual stage i over N images: a ConvArgs without pointers or tiles
static_assert(kStageFilters[0] % 64 == 0 && kStageFilters[1] % 64 == 0 && kStageFilters[2] % 64 == 0 && kStageFilters[3] % 64 == 0,
              "conv channels unsupported (Cin % 32, Cout % 64)");
static ConvArgs conv_geom(const TrunkDims& d, int N, int i, int k) {
  ConvArgs a{};
  a.N = N; a.Ho = d.h[2 + i]; a.Wo = d.w[2 + i]; a.Cout = kStageFilters[i];
  a.Hi = k == 1 ? a.Ho : d.h[1 + i]; a.Wi = k == 1 ? a.Wo : d.w[1 + i];
  a.Cin = k == 1 ? a.Cout : (i == 0 ? 64 : kStageFilters[i - 1]);
  a.KH = a.KW = k == 2 ? 1 : 3; a.stride = k == 1 ? 1 : kStageStride[i];
  a.pad = std::max((a.Ho - 1) * a.stride + a.KH - a.Hi, 0) / 2;
  a.padw = std::max((a.Wo - 1) * a.stride + a.KW - a.Wi, 0) / 2;
  a.M = N * a.Ho * a.Wo; a.P = a.Ho * a.Wo;
  return a;
}

// shapes the row-slab kernel takes: stride-1 3x3 convs with 64 or 128 output channels on 32- or 16-pixel-wide maps
static bool rowslab_shape_ok(const ConvArgs& a) {
  return a.KH == 3 && a.stride == 1 && a.Cout <= 128 && a.Cin % 16 == 0 && a.Hi == a.Ho &&
         a.Wi == a.Wo && (a.Wo == 32 || a.Wo == 16) && a.Ho % (256 / a.Wo) == 0 && (long)a.N * a.Hi * a.Wi * a.Cin < (1L << 31);
}
// the fused epilogue's wait needs more than 8 (G - 1) co-resident workgroups (see FuseArgs); demand twice that of the
// `resident` workgroups the stream can hold at ONE per CU, else run the separate elementwise pass
static bool fused_can_wait(int resident, int G) { return resident >= 16 * (G - 1) + 1; }

// Kernel, tile configuration and epilogue of one conv.  `fuse`: the pass asks for the fused GroupNorm epilogue (conv0 / conv1);
// `raw`: the input is conv_init's raw pooled tensor; `proj`: the block's projection is offered to this conv0 (same input,
// stride and output shape).
static TrunkPlan::L plan_conv(const ConvArgs& a, bool dma, bool zero_page, bool fuse, int resident, bool raw, bool proj) {
  TrunkPlan::L l;
  // tile configuration of the register-staged / LDS-DMA kernels: 0 = 128x128, 1 = 256x64 (Cout == 64), 4 = 128x64 with three
  // chunks in flight (fewer than 512 128x128 tiles but at least 512 128x64 ones; measured per layer at B/2, B/4, B/8),
  // 2 = 64x64 with three chunks in flight (small M: one rank's share of a data-parallel batch)
  int cfg = a.Cout >= 128 ? 0 : 1;
  if (cfg == 0 && (long)cdiv(a.M, 128) * (a.Cout / 128) < 512) cfg = 2;
  if (cfg == 2 && (long)cdiv(a.M, 128) * (a.Cout / 64) >= 512) cfg = 4;
  const int wrows = cfg == 2 ? 32 : 64;
  // how a wave's rows relate to images (GroupNorm statistics in the epilogue): 0 = a wave lies in one image, 1 / 2 = images
  // of 32 / 16 pixels, 3 = none of these: statistics by gn_stats_kernel_b after the conv
  int pmode = (a.P % wrows == 0) ? 0 : (a.P == 32 ? 1 : (a.P == 16 ? 2 : 3));
  if (cfg == 2 && pmode == 1) pmode = 3;
  const bool fits32 = (long)a.N * a.Hi * a.Wi * a.Cin * 4 < (1L << 32);   // 32-bit byte offsets into the input
  // row-slab kernels: stride-1 3x3 convs with 64 or 128 output channels on 32- or 16-pixel-wide maps (stage 0, b1_conv1), weights (and,
  // for a split8 input, the slab) by LDS-DMA
  const bool slab_ok = rowslab_shape_ok(a) && a.pad == 1 && a.padw == 1 && dma && (raw || (zero_page && fits32));
  // LDS-DMA kernel: everything else with at least 512 128-row tiles
  const bool dma_ok = (cfg == 0 || cfg == 4) && a.Cin % 32 == 0 && zero_page && dma && fits32;
  if (slab_ok) {
    l.kern = 'S'; l.cfg = 9; l.raw = raw;
    const int tiles_n = a.Cout / 64;
    if (fuse && a.P == 256) {
      l.fused = 2;   // LOCAL: a 256 x 64 tile = one whole image over complete groups, nothing to exchange and nobody to wait for
    } else if (fuse && a.P % 256 == 0 && fused_can_wait(resident, a.P / 256 * tiles_n)) {
      l.fused = 1; l.expected = a.P / 256; l.group = a.P / 256 * tiles_n;
    }
    // anti-phase start: 5 x s_sleep(127) ~ 20 us ~ half a tile of the stage-0 convs.  Same-call A/B (profiles/r04_ab_rs_stagger.txt):
    // pipelined step 2.5762 / 2.5747 -> 2.5523 / 2.5489 ms with 5; 3 and 8 (a quarter / three quarters of a tile) gave nothing
    l.stagger = (l.fused && a.M / 256 * tiles_n >= 1024) ? 5 : 0;
  } else if (dma_ok) {
    l.kern = 'D'; l.cfg = cfg;
    const int tn = cfg == 0 ? 2 : 1, tiles_n = a.Cout / (64 * tn);
    if (pmode == 1 && cfg == 4) pmode = 3;
    // (the exchange is among the row tiles of ONE column tile: a GroupNorm group must not be wider than the tile)
    if (fuse && pmode == 0 && a.P % 128 == 0 && a.Cout / kGnGroups <= 64 * tn && fused_can_wait(resident, a.P / 128 * tiles_n)) {
      l.fused = 1; l.expected = a.P / 128; l.group = a.P / 128 * tiles_n;
    } else if (fuse && pmode == 0 && a.P == 64 && a.M % 128 == 0 && tn == 2 && a.Cout / kGnGroups == 64) {
      l.fused = 2;   // LOCAL: a wave = one (image, group), no exchange
    } else if (fuse && pmode == 2 && a.P == 16 && a.M % 128 == 0 && tn == 2 && a.Cout / kGnGroups == 128) {
      l.fused = 2;   // LOCAL, stage 3: a 128 x 128 tile = eight whole images of one group (dma_tile_epilogue)
    }
    // projection pixel == conv0's tap (0, 0): pad 0 on both axes ("SAME" padding of an even extent at stride 2)
    l.proj = proj && pmode != 3 && a.KH == 3 && a.stride == 2 && a.pad == 0 && a.padw == 0;
  } else {
    l.kern = 'R'; l.cfg = cfg;
  }
  l.pmode = pmode;
  l.pad = a.pad; l.padw = a.padw;
  return l;
}

// The whole plan of a split-fp16 pass over N images: `dma` / `zero` of the packed weights, the blocks that have projections,
// the workgroups the stream can hold (resident_workgroups) and the pass switches.  No HIP call, no environment: a pass issued
// in pieces launches what its first piece planned.
static int plan_pass(TrunkPlan& p, const TrunkDims& d, int N, const TrunkPacked& pk, const bool (&has_proj)[kTrunkStages], int resident,
                     bool fuse, bool proj_fuse) {
  p = TrunkPlan{};
  p.images = N; p.fuse = fuse;
  // FAST STAGE-0 INPUT: with many images conv_init completes the pooling itself (whole-image chunks) and block 0 consumes the
  // raw pooled tensor directly -- b0_conv0 applies GroupNorm + ReLU + split while staging its slabs (row-slab RAWIN), b0_conv1's
  // fused epilogue rebuilds the residual from the same raw tensor (mode 4): no elementwise pass over the pooled tensor.
  // Needs: full 16x16 conv_init tiles, at least 2 images per persistent workgroup, block 0 on the row-slab kernel with its
  // fused epilogue available.
  const bool fuse_pool = d.h[0] % 16 == 0 && d.w[0] % 16 == 0;   // full 16 x 16 conv_init tiles: pooling fused into conv_init
  const bool complete_pool = fuse_pool && N >= 512 && N % 512 == 0;
  p.pool = complete_pool ? 2 : (fuse_pool ? 1 : 0);
  const ConvArgs b0 = conv_geom(d, N, 0, 0);
  p.raw_b0 = complete_pool && fuse && !has_proj[0] && rowslab_shape_ok(b0) && b0.Cin <= 128 && pk.blk[0][0].dma && pk.blk[0][1].dma &&
             b0.P % 256 == 0 && fused_can_wait(resident, b0.P / 256 * (b0.Cout / 64));
  for (int i = 0; i < kTrunkStages; ++i) {
    TrunkPlan::L* l = p.conv[i];
    const bool raw = i == 0 && p.raw_b0;
    l[0] = plan_conv(conv_geom(d, N, i, 0), pk.blk[i][0].dma, pk.zero, fuse, resident, raw, has_proj[i] && proj_fuse && pk.blk[i][2].dma);
    if (l[0].proj) {
      l[2] = l[0];
      l[2].kern = 'F'; l[2].fused = 0;
    } else if (has_proj[i]) {
      l[2] = plan_conv(conv_geom(d, N, i, 2), pk.blk[i][2].dma, pk.zero, false, resident, false, false);
    }
    l[1] = plan_conv(conv_geom(d, N, i, 1), pk.blk[i][1].dma, pk.zero, fuse, resident, false, false);
    SERL_REQUIRE(!raw || (l[0].kern == 'S' && l[0].fused && l[1].fused),
                 "block 0 was planned on the fused row-slab path");
  }
  return SERL_OK;
}

template <int WM, int WN, int TM, int TN, int DEEP>
static void launch_igemm(ConvArgsB ab, int pmode, hipStream_t stream) {
  constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
  ab.c.tiles_m = cdiv(ab.c.M, BM); ab.c.tiles_n = ab.c.Cout / BN;
  const dim3 grid(ab.c.tiles_m * ab.c.tiles_n), block(256);
  const size_t lds = (size_t)2 * (2 * BM * 64 + 2 * BN * 64);
  if (pmode == 0) hipLaunchKernelGGL((conv_igemm_f16x3_kernel<WM, WN, TM, TN, 0, DEEP>), grid, block, lds, stream, ab);
  else if (pmode == 1) hipLaunchKernelGGL((conv_igemm_f16x3_kernel<WM, WN, TM, TN, 1, DEEP>), grid, block, lds, stream, ab);
  else if (pmode == 2) hipLaunchKernelGGL((conv_igemm_f16x3_kernel<WM, WN, TM, TN, 2, DEEP>), grid, block, lds, stream, ab);
  else hipLaunchKernelGGL((conv_igemm_f16x3_kernel<WM, WN, TM, TN, 3, DEEP>), grid, block, lds, stream, ab);
}
template <int TN, bool PROJ>
static void launch_dma(ConvArgsB ab, int pmode, const uint8_t* zero_page, const ConvProjB& pj, hipStream_t stream) {
  ab.c.tiles_m = cdiv(ab.c.M, 128); ab.c.tiles_n = ab.c.Cout / (64 * TN);
  const dim3 grid(ab.c.tiles_m * ab.c.tiles_n), block(256);
  const size_t lds = (size_t)4 * (128 * 64 + 64 * TN * 64);   // ring of four 16-channel slots
  if (pmode == 0) hipLaunchKernelGGL((conv_dma_f16x3_kernel<TN, 0, PROJ>), grid, block, lds, stream, ab, zero_page, pj);
  else if (pmode == 1) hipLaunchKernelGGL((conv_dma_f16x3_kernel<TN, 1, PROJ>), grid, block, lds, stream, ab, zero_page, pj);
  else if (pmode == 2 || PROJ) hipLaunchKernelGGL((conv_dma_f16x3_kernel<TN, 2, PROJ>), grid, block, lds, stream, ab, zero_page, pj);
  else if constexpr (!PROJ) hipLaunchKernelGGL((conv_dma_f16x3_kernel<TN, 3, false>), grid, block, lds, stream, ab, zero_page, pj);
}
// Launches one conv as `l` planned it.  `a`: conv_geom plus the input (with its GroupNorm for a raw input), output and
// statistics; `fz`: the fused epilogue's arguments (used if l.fused); `pj`: the projection riding on conv0 (used if l.proj).
static int launch_conv_f16x3(const char* tag, const TrunkPlan::L& l, const ConvArgs& a, PackedConvWeights w, const FuseArgs& fz,
                             const ConvProjB& pj, const uint8_t* zero_page, hipStream_t stream) {
  ConvArgsB ab{};
  ab.c = a;
  ab.whi = w.hi; ab.wlo = w.lo; ab.winv = w.inv; ab.wdma = w.dma; ab.K = a.KH * a.KW * a.Cin;
  ab.wprio = trunk_wave_prio(a.N);
  ab.stagger = l.stagger;
  if (l.fused) { ab.fz = fz; ab.fz.expected = l.expected; ab.fz.group = l.group; }
  // (the projection kernels are compiled without the residual epilogues: conv_dma_f16x3_kernel)
  SERL_REQUIRE(!l.proj || ab.fz.mode < 2, "%s: a conv with a fused projection cannot take a residual (mode %d)", tag, (int)ab.fz.mode);
  {
    ProfScope prof(tag, stream);
    if (l.kern == 'S') {
      // a fused launch stores ROW-major (rowtile_epilogue_t; same-call pipelined step 2.494 / 2.497 -> 2.474 / 2.471 ms against the C-layout
      // fused epilogue it replaced, profiles/r05_ab_epilogue_t.txt), an unfused one stores the raw tile
      ab.c.tiles_m = a.M / 256; ab.c.tiles_n = a.Cout / 64;
      const dim3 grid(ab.c.tiles_m * ab.c.tiles_n), block(256);
      if (l.raw)   // b0_conv0 on conv_init's raw pooled output: GroupNorm + ReLU + split while the slab is staged, weights by LDS-DMA
        hipLaunchKernelGGL(conv3x3_rowslab_f16x3_kernel, grid, block, (size_t)kRowslabLds, stream, ab);
      // split8 input (b0_conv1, b1_conv1): slab and weights by LDS-DMA (same-call -2.2 % of the pipelined step against the
      // register-staged kernel it replaced in round 5, profiles/r05_ab_slab_dma.txt)
      else if (l.fused) hipLaunchKernelGGL(conv3x3_slabdma_f16x3_kernel<true>, grid, block, (size_t)kSlabDmaLds, stream, ab, zero_page);
      else hipLaunchKernelGGL(conv3x3_slabdma_f16x3_kernel<false>, grid, block, (size_t)kSlabDmaLds, stream, ab, zero_page);
    } else if (l.kern == 'D') {
      // (tile configuration 0: 128 x 128, 4: 128 x 64)
      if (l.proj) {
        if (l.cfg == 0) launch_dma<2, true>(ab, l.pmode, zero_page, pj, stream);
        else launch_dma<1, true>(ab, l.pmode, zero_page, pj, stream);
      } else if (l.cfg == 0) launch_dma<2, false>(ab, l.pmode, zero_page, ConvProjB{}, stream);
      else launch_dma<1, false>(ab, l.pmode, zero_page, ConvProjB{}, stream);
    } else {
      if (l.cfg == 0) launch_igemm<2, 2, 2, 2, 0>(ab, l.pmode, stream);
      else if (l.cfg == 1) launch_igemm<4, 1, 2, 2, 0>(ab, l.pmode, stream);
      else if (l.cfg == 4) launch_igemm<2, 2, 2, 1, 3>(ab, l.pmode, stream);
      else launch_igemm<2, 2, 1, 1, 3>(ab, l.pmode, stream);
      // (K-split of the small-M convs -- 2..8 workgroups per 64x64 tile -- was built twice: in round 3 with slabs reduced by the
      //  statistics kernel (halved b3_conv1 at a per-rank batch of 32, but the step got slower), in round 4 summed by the last
      //  arriver inside the launch (kernels faster while the split launch fitted one round of the chip, the B/8 step 0.765 ->
      //  0.773 ms: there the update chain bounds the step).  Removed; profiles/README.md round 4.)
    }
  }
  SERL_HIP(hipGetLastError());
  if (l.pmode == 3) {
    hipLaunchKernelGGL(gn_stats_kernel_b, dim3(a.N * kGnGroups), dim3(256), 0, stream, a.out, a.stats, a.P, a.Cout);
    SERL_HIP(hipGetLastError());
  }
  return SERL_OK;
}

// Zeroes the statistics (of the unfused layers: a fused launch writes none) and the tickets of a pass -- and, before a workspace's
// first pass, its exchange records -- with SYSTEM-scope (write-through, sc0 sc1) 16-byte stores.
// Everything that touches these words afterwards is a memory-side access (stats_flush, fused_tile, gnx_publish / gnx_collect),
// so the zeroes must be AT the memory side too and no cache may keep a copy: a plain-store zeroing kernel (round 2, reverted
// after one unexplained parity failure) leaves the zeroed lines dirty in the L2 of whichever XCD ran the store until that
// L2 writes them back -- ordered against the next kernel only by the launch boundary's cache maintenance, i.e. outside the
// "memory-side accesses only" rule the fused epilogues rely on.  hipMemsetAsync (the blit kernel, 19 us for 1.3 MB) has the
// same property; this kernel takes ~3 us and keeps the rule by construction.
__global__ __launch_bounds__(256) void zero_sys_kernel(void* p, long n16) {
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(p, 0, 0x7fffffff, 0x00020000);
  const u32x4 z = {0u, 0u, 0u, 0u};
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n16; i += (long)gridDim.x * 256)
    __builtin_amdgcn_raw_buffer_store_b128(z, r, (int)(i * 16), 0, 17 /* sc0 | sc1 */);
}

// ONE fused pass at a time per process.  The fused GroupNorm epilogues WAIT for other workgroups of their launch, and their
// forward-progress argument (FuseArgs) counts on every resident workgroup that waits belonging to THIS launch.  Two agents
// whose passes run concurrently on two streams break that: the CUs can fill up with waiters of both launches while the
// workgroups they wait for cannot start -- a deadlock the spin bound turns into a trap (found by round 4's 2000-step stress
// test, which keeps a second and a third agent's passes running on other streams).  A pass therefore claims the fused path
// only if the previous fused pass was issued on the same stream (in order: no overlap) or has completed (event query);
// otherwise it runs the separate elementwise passes (same results, ~10 % slower, no waiting of any kind).  Passes of OTHER
// processes on the same GPU cannot be seen from here: run one learner process per GPU, or set SERL_GN_FUSE=0.
static std::mutex g_fused_mu;
static hipStream_t g_fused_stream = nullptr;
static hipEvent_t g_fused_done = nullptr;
static bool g_fused_any = false, g_fused_open = false;   // open: a pass issued in pieces has not issued its last piece yet
static bool claim_fused_pass(hipStream_t stream) {
  std::lock_guard<std::mutex> lk(g_fused_mu);
  if (g_fused_any && g_fused_stream != stream &&
      (g_fused_open || (g_fused_done && hipEventQuery(g_fused_done) == hipErrorNotReady))) return false;
  (void)hipGetLastError();
  g_fused_stream = stream;
  g_fused_any = g_fused_open = true;
  return true;
}
static void fused_pass_issued(hipStream_t stream) {
  std::lock_guard<std::mutex> lk(g_fused_mu);
  if (g_fused_stream != stream) return;
  g_fused_open = false;
  if (!g_fused_done && hipEventCreateWithFlags(&g_fused_done, hipEventDisableTiming) != hipSuccess) { g_fused_done = nullptr; return; }
  (void)hipEventRecord(g_fused_done, stream);
}

// Trunk forward in split-fp16 arithmetic.  Activations between kernels live in the split16 layout;
// raw conv outputs (pre-GroupNorm) and the final features stay fp32.
int trunk_forward_f16x3(const TrunkWeights& w, TrunkWorkspace& ws, TrunkPacked& pk, const uint8_t* frames, int N,
                        float* feats_out, hipStream_t stream, int stage_begin, int stage_end) {
  // [stage_begin, stage_end]: -1 = conv_init + pool, 0..3 = residual stages; a pass may be issued in consecutive pieces
  // (the intermediate activations live in the workspace), which lets the caller put an event between them
  const TrunkDims& d = ws.d;
  const TrunkPlan& plan = ws.plan;
  auto stats_of = [&](int layer) { return ws.stats + (size_t)layer * ws.max_images * kGnGroups * 2; };
  int rc;
  if (stage_begin < 0) {
    // the pass switches, read once per pass (tests flip them inside one process): fused GroupNorm epilogues (SERL_GN_FUSE, and
    // the claim), the projections riding on conv0 (SERL_PROJ_FUSE).  FUSED PROJECTION (default; SERL_PROJ_FUSE=0 restores the
    // separate launch): conv0's workgroups compute the block's projection tile too -- no projection launch, one more pass over
    // tap (0, 0) of an input tile that conv0 fetches anyway.  Same-call A/B (profiles/r05_call1): pipelined step 2.557 -> 2.535
    // ms, serial 3.000 -> 2.970; tests/test_agent_gpu.py::test_fused_projection
    const char* gf = getenv("SERL_GN_FUSE");
    const char* pf = getenv("SERL_PROJ_FUSE");
    const bool fuse = !(gf && gf[0] == '0') && claim_fused_pass(stream);
    const bool has_proj[kTrunkStages] = {w.blk[0].proj != nullptr, w.blk[1].proj != nullptr, w.blk[2].proj != nullptr,
                                         w.blk[3].proj != nullptr};
    const int resident = fuse ? resident_workgroups(stream) : 0;   // (only the fused epilogues wait for other workgroups)
    if ((rc = plan_pass(ws.plan, d, N, pk, has_proj, resident, fuse, !(pf && pf[0] == '0')))) return rc;
    auto zero_sys = [&](void* p, size_t bytes) -> int {
      for (size_t off = 0; off < bytes; off += (size_t)1 << 30) {   // (32-bit buffer offsets: 1 GiB per launch)
        const long n16 = (long)(std::min(bytes - off, (size_t)1 << 30) / 16);
        hipLaunchKernelGGL(zero_sys_kernel, dim3((unsigned)std::min<long>(cdiv(n16, 256), 512)), dim3(256), 0, stream,
                           (void*)((uint8_t*)p + off), n16);
        SERL_HIP(hipGetLastError());
      }
      return SERL_OK;
    };
    // statistics + tickets (both regions are multiples of 256 bytes: trunk_layout)
    if ((rc = zero_sys(ws.stats, ws.stats_sync_bytes))) return rc;
    // the pass epoch = the tag of this pass's granules (gn_exchange.h); the records are zeroed only when the rule says so
    const GnxEpoch ep = gnx_next_epoch(ws.epoch);
    if (ep.clear && (rc = zero_sys(ws.rec, ws.rec_bytes))) return rc;
    ws.epoch = ep.epoch;
  } else {
    SERL_REQUIRE(plan.images == N, "trunk pass piece over %d images continues a pass planned for %d", N, plan.images);
  }
  auto fuse_of = [&](int layer, int mode) {
    FuseArgs f{};
    f.mode = mode;
    f.ticket = ws.tickets + (size_t)layer * kSyncTickets;
    f.rec = ws.rec + ws.rec_off[layer] * kGnxGranules;
    f.epoch = ws.epoch;
    return f;
  };
  const GnRef gn_init = gn_ref(stats_of(0), w.gn_init_s, w.gn_init_b, d.h[0] * d.w[0], 64);
  if (stage_begin < 0) {
    if ((rc = launch_conv_init_f16x3(frames, PackedConvWeights{pk.init.hi, pk.init.lo, pk.init.inv}, ws.raw_init, stats_of(0), N, d.H,
                                     d.W, d.h[0], d.w[0], stream, plan.pool ? w.gn_init_s : nullptr, fuse_of(0, 0).ticket,
                                     plan.pool == 2))) return rc;
    if (plan.raw_b0) {
      // nothing: block 0 reads ws.raw_init (the completed pooled tensor) itself
    } else if (plan.pool == 2) {
      const long tot = (long)N * d.h[1] * d.w[1] * 16;
      ProfScope prof("gn_relu_maxpool", stream);
      hipLaunchKernelGGL(gn_relu_split_kernel, dim3(cdiv(tot, 256)), dim3(256), 0, stream, ws.raw_init, gn_init,
                         reinterpret_cast<uint4*>(ws.pool), N, d.h[1] * d.w[1], 64);
      SERL_HIP(hipGetLastError());
    } else if (plan.pool == 1) {
      const long tot = (long)N * d.h[1] * (d.w[1] / 4) * 16;   // 4 pooled pixels per thread (Wo % 16 == 0)
      const int ty = d.h[0] / 16, tx = d.w[0] / 16;
      const float* pooled = ws.raw_init;
      const float* frows = pooled + (size_t)N * d.h[1] * d.w[1] * 64;
      const float* fcols = frows + (size_t)N * ty * d.w[0] * 64;
      ProfScope prof("gn_relu_maxpool", stream);
      hipLaunchKernelGGL(pool_finish_split_kernel, dim3(cdiv(tot, 256)), dim3(256), 0, stream, pooled, frows, fcols, gn_init,
                         reinterpret_cast<uint4*>(ws.pool), N, d.h[0], d.w[0], ty, tx);
      SERL_HIP(hipGetLastError());
    } else {
      const long tot = (long)N * d.h[1] * d.w[1] * 16;
      ProfScope prof("gn_relu_maxpool", stream);
      hipLaunchKernelGGL(gn_relu_maxpool_split_kernel, dim3(cdiv(tot, 256)), dim3(256), 0, stream, ws.raw_init, gn_init,
                         reinterpret_cast<uint4*>(ws.pool), N, d.h[0], d.w[0], d.h[1], d.w[1], 64);
      SERL_HIP(hipGetLastError());
    }
  }
  // one residual stage as planned: conv0 (+ projection), GroupNorm + ReLU + split8 of conv0, conv1, block output -- the
  // elementwise passes only where the conv before them has no fused epilogue
  auto run_stage = [&](int i) -> int {
    const int f = kStageFilters[i], P = d.h[2 + i] * d.w[2 + i];
    const int l0 = 1 + 3 * i, l1 = 2 + 3 * i, lp = 3 + 3 * i;
    const TrunkWeights::Block& bw = w.blk[i];
    const TrunkWorkspace::B& t = ws.blk[i];
    const TrunkPlan::L* pl = plan.conv[i];
    const bool has_proj = bw.proj != nullptr, last = i == kTrunkStages - 1;
    const float* x = i == 0 ? ws.pool : ws.blk[i - 1].out;   // split16
    float* const feats = last ? feats_out : nullptr;
    auto pw = [&](int k) { return PackedConvWeights{pk.blk[i][k].hi, pk.blk[i][k].lo, pk.blk[i][k].inv, pk.blk[i][k].dma}; };
    auto args = [&](int k, const float* in, float* out, int layer) {
      ConvArgs a = conv_geom(d, N, i, k);
      a.in = in; a.out = out; a.stats = stats_of(layer);
      return a;
    };
    int rc;
    // conv0: GroupNorm + ReLU + split8 in its epilogue where planned, else gn_relu_split below
    ConvArgs a0 = args(0, x, t.raw0, l0);
    if (pl[0].raw) { a0.in = ws.raw_init; a0.in_gn = gn_init; }
    FuseArgs fz0 = fuse_of(l0, 1);
    fz0.gn = gn_ref(stats_of(l0), bw.gn0_s, bw.gn0_b, P, f);
    fz0.out_split = reinterpret_cast<uint8_t*>(t.norm0);
    ConvProjB pj{};
    if (pl[0].proj) { pj.wdma = pk.blk[i][2].dma; pj.winv = pk.blk[i][2].inv; pj.out = t.rawp; pj.stats = stats_of(lp); }
    if ((rc = launch_conv_f16x3(kConvTags[i][0], pl[0], a0, pw(0), fz0, pj, pk.zero, stream))) return rc;
    if (has_proj && !pl[0].proj)
      if ((rc = launch_conv_f16x3(kConvTags[i][2], pl[2], args(2, x, t.rawp, lp), pw(2), FuseArgs{}, ConvProjB{}, pk.zero, stream))) return rc;
    const long tot = (long)N * P * (f / 4);
    if (!pl[0].fused) {
      ProfScope prof("gn_relu_split", stream);
      hipLaunchKernelGGL(gn_relu_split_kernel, dim3(cdiv(tot, 256)), dim3(256), 0, stream, t.raw0, fz0.gn,
                         reinterpret_cast<uint4*>(t.norm0), N, P, f);
      SERL_HIP(hipGetLastError());
    }
    // conv1: block output in its epilogue where planned, else block_out below.  (The last block's conv1 writes the trunk's
    // features: plain fp32 -- out_f32 -- where its kernel has a fused epilogue for the shape: the LOCAL stage-3 form of
    // dma_tile_epilogue since round 6.)
    FuseArgs fz1 = fuse_of(l1, has_proj ? 3 : (pl[0].raw ? 4 : 2));
    fz1.gn = gn_ref(stats_of(l1), bw.gn1_s, bw.gn1_b, P, f);
    fz1.out_split = last ? nullptr : reinterpret_cast<uint8_t*>(t.out);
    fz1.out_f32 = feats;
    if (has_proj) {
      fz1.res_raw = t.rawp;
      fz1.res_gn = gn_ref(stats_of(lp), bw.gnp_s, bw.gnp_b, P, f);
    } else if (pl[0].raw) {
      fz1.res_raw = ws.raw_init;
      fz1.res_gn = gn_init;
    } else {
      fz1.res_split = reinterpret_cast<const uint8_t*>(x);
    }
    if ((rc = launch_conv_f16x3(kConvTags[i][1], pl[1], args(1, t.norm0, t.raw1, l1), pw(1), fz1, ConvProjB{}, pk.zero, stream))) return rc;
    if (!pl[1].fused) {
      ProfScope prof("block_out", stream);
      hipLaunchKernelGGL(block_out_split_kernel, dim3(cdiv(tot, 256)), dim3(256), 0, stream, t.raw1, fz1.gn,
                         has_proj ? nullptr : reinterpret_cast<const uint4*>(x), has_proj ? t.rawp : nullptr,
                         has_proj ? fz1.res_gn : GnRef{}, last ? nullptr : reinterpret_cast<uint4*>(t.out), feats, N, P, f);
      SERL_HIP(hipGetLastError());
    }
    return SERL_OK;
  };
  // (A DEPTH-FIRST schedule -- stages 0 and 1 issued chunk by chunk over 128 / 256 / 512 images with every chunk-local tensor in one
  // re-used window sized for the 256 MiB Infinity Cache -- was built and measured in round 5: correct, and SLOWER in every
  // configuration (pipelined step 2.557 -> 2.638 / 2.739 / 3.030 ms at 512 / 256 / 128 images per chunk, serial 3.000 -> 3.109):
  // the kernels lose more at small M than cache-resident tensors give back.  Removed; profiles/README.md, r05_call1.)
  for (int i = std::max(stage_begin, 0); i <= stage_end; ++i)
    if ((rc = run_stage(i))) return rc;
  if (plan.fuse && stage_end == kTrunkStages - 1) fused_pass_issued(stream);
  return SERL_OK;
}

}  // namespace serl
