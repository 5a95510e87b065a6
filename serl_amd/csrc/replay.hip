// HBM-resident memory-efficient replay buffer for SERL on MI355X (gfx950).
//
// Host side: replay_index.h holds the reference's slot bookkeeping and index sampler (no HIP, tested on the CPU); this
// file stages host data through pinned rings, orders the streams and launches the kernels.
// Device side: one fused kernel = sample gather + concat_batches + _unpack + DrQ random shift
// (K2+K3+K4).  It is HBM-bound u8 traffic: every source frame row is pulled once with 16-byte
// coalesced loads into LDS, shifted/clamped out of LDS, and written once with 16-byte stores.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "common.h"
#include "prof.h"
#include "replay_batch.h"
#include "replay_index.h"
#include "stack_index.h"

namespace serl {

thread_local char g_err[512] = {0};
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

constexpr int kRing = 8;           // staging slots for per-call index/crop parameters
constexpr int kInsRing = 32;       // pinned staging slots for inserted transitions (one slot write each)
constexpr int kRowsPerBlock = 32;  // output rows per workgroup in the gather/crop kernel
constexpr int kMaxStack = 4;       // most frames per observation the crop kernels and the agent serve (serl_agent_cfg.num_stack)
constexpr size_t kXferChunk = (size_t)8 << 20;  // bytes per pinned staging buffer of the snapshot export / import (two of them)
constexpr int kBatRing = 2;                     // staging slots of the batched insert, pinned and device: one launch each
constexpr size_t kBatBudget = (size_t)2 << 20;  // bytes per such slot (it always holds at least one entry)
constexpr int kHandOverUs = 100;                // longest a batched insert stands back for waiting readers between two groups

// A ring of `n` pinned host slots (and, if asked for, as many device slots) with one event per slot.  acquire() hands out the
// next slot, first waiting for the work that last used it if the ring has wrapped; mark() records that work's end.  The owner
// serialises the calls (a mutex), so the slot between an acquire and its mark is `cur`.
struct StageRing {
  uint8_t* host = nullptr;
  uint8_t* dev = nullptr;
  size_t slot_bytes = 0;
  int n = 0, next = 0, cur = 0;
  hipEvent_t done[kInsRing] = {nullptr};
  bool used[kInsRing] = {false};

  int init(int n_slots, size_t bytes, bool with_dev) {
    n = n_slots; slot_bytes = bytes;
    SERL_HIP(hipHostMalloc((void**)&host, slot_bytes * n, hipHostMallocDefault));
    if (with_dev) SERL_HIP(hipMalloc((void**)&dev, slot_bytes * n));
    for (int s = 0; s < n; ++s) SERL_HIP(hipEventCreateWithFlags(&done[s], hipEventDisableTiming));
    return SERL_OK;
  }
  void destroy() {  // tolerates a half-built ring
    if (host) (void)hipHostFree(host);
    if (dev) (void)hipFree(dev);
    for (int s = 0; s < kInsRing; ++s)
      if (done[s]) (void)hipEventDestroy(done[s]);
  }
  int acquire() {
    cur = next;
    next = (cur + 1) % n;
    if (used[cur]) SERL_HIP(hipEventSynchronize(done[cur]));  // ring wrapped: that work is long done
    return SERL_OK;
  }
  int mark(hipStream_t stream) {
    SERL_HIP(hipEventRecord(done[cur], stream));
    used[cur] = true;
    return SERL_OK;
  }
  uint8_t* h() const { return host + (size_t)cur * slot_bytes; }
  uint8_t* d() const { return dev + (size_t)cur * slot_bytes; }
};

}  // namespace serl

struct serl_rb {
  int device = 0;
  int n_cam = 0, H = 0, W = 0, C = 0, T = 1, S = 0, A = 0;
  int rec_len = 0;  // floats per record: [state T*S | next_state T*S | action A | reward | mask | done]
  size_t frame_bytes = 0;
  uint8_t* frames[SERL_MAX_CAMS] = {nullptr};  // device, [cap][H*W*C] each
  float* rec = nullptr;                        // device, [cap][rec_len]
  serl::ReplayIndex ix;  // host bookkeeping (memory_efficient_replay_buffer.py); guarded by `mu`
  std::mutex mu;
  // snapshot export (serl_rb_export_slots): while `busy`, inserts and other exports / imports wait on `idle` with the mutex
  // released -- index draws and gathers only take the mutex and go on.  The two pinned staging buffers are made at the first use.
  std::condition_variable idle;
  bool busy = false;
  uint8_t* xfer_host = nullptr;
  hipEvent_t xfer_done[2] = {nullptr, nullptr};
  // stream/event plumbing
  hipStream_t copy_stream = nullptr;
  // one "last gather" event per stream that gathers from this buffer (the learner's update stream, its prefetch side
  // stream, ...): an overwriting insert waits for ALL of them
  static constexpr int kGatherStreams = 4;
  hipEvent_t gather_ev[kGatherStreams] = {nullptr, nullptr, nullptr, nullptr};
  hipStream_t gather_stream[kGatherStreams] = {nullptr, nullptr, nullptr, nullptr};
  bool gather_used[kGatherStreams] = {false, false, false, false};
  bool gather_pend[kGatherStreams] = {false, false, false, false};
  int gather_rr = 0;
  bool gather_pending = false;
  // inserts are staged through a pinned ring (slot = padded record + one frame per camera) and copied asynchronously on
  // copy_stream: the caller's thread (the actor-facing server thread of data_store.py:104-106) holds the mutex for a host
  // memcpy only, never for a stream synchronisation, so it cannot stall the learner thread's sample_indices / gather
  serl::StageRing ins;
  hipEvent_t last_insert = nullptr;
  bool insert_pending = false;
  serl::StageRing stage;  // per-call parameter staging (pinned host + device)
  // batched inserts (serl_rb_insert_batch): replay_batch.h groups the slot operations of a payload into launches; a launch is
  // staged in one slot of `bat` -- its entries (one slot write each, laid out like a slot of `ins`: the record padded to
  // rec_pad bytes, then one frame per camera), then its op table -- and costs one H2D copy and one insert_scatter_kernel on
  // copy_stream.  The ring is made at the first batched call.
  size_t rec_pad = 0, entry_bytes = 0;
  serl::StageRing bat;
  bool bat_taken = false;  // the launch being built has its slot of `bat`
  serl::BatchPlan plan;
  int64_t stats[4] = {0, 0, 0, 0};  // serl_rb_insert_stats
  // index draws and gathers that wait for `mu` or hold it (Reader below).  Between two of its groups a batched insert stands
  // back while this is not zero, for at most kHandOverUs: unlocking alone lets nobody in, the inserting thread has the mutex
  // back before a thread it woke gets to run.  The wait is bounded, so readers that overlap without end cannot starve inserts.
  std::atomic<int> readers{0};
};

namespace serl {

// ---------------------------------------------------------------------------------------------
// device kernels
// ---------------------------------------------------------------------------------------------
struct GatherArgs {
  const uint8_t* frames[SERL_MAX_BUFFERS][SERL_MAX_CAMS];
  const float* rec[SERL_MAX_BUFFERS];
  const int64_t* idx[SERL_MAX_BUFFERS];  // device, per buffer
  int64_t cap[SERL_MAX_BUFFERS];
  int count0;                            // samples [0,count0) come from buffer 0
  int batch, n_cam, H, W, C, S, A, rec_len;   // S = floats of one observation's state (T * state_dim of the store)
  int T;                     // frames per observation (num_stack)
  const int32_t* crop_obs;   // device [batch*T][2] or nullptr
  const int32_t* crop_next;  // device [batch*T][2] or nullptr
  uint8_t* out_frames;       // [2][n_cam][batch][T][H][W][C]
  float* out_state;          // [2][batch][S]
  float* out_action;         // [batch][A]
  float* out_reward;
  float* out_mask;
  uint8_t* out_done;
  int n_frame_blocks;
  // packed mode (serl_crop_packed_stacked): source is dev_packed[c] u8[batch][T+1][H][W][C]
  const uint8_t* packed[SERL_MAX_CAMS];
  int from_packed;
};

struct PackedArgs {
  const uint8_t* frames[SERL_MAX_CAMS];
  const float* rec;
  const int64_t* idx;
  int batch, n_cam, T, TS, A, rec_len;
  int64_t cap;
  size_t fbytes;
  uint8_t* out_frames[SERL_MAX_CAMS];  // [batch][T+1][fbytes]
  float *out_state, *out_next_state, *out_action, *out_reward, *out_mask;
  uint8_t* out_done;
  int n_frame_blocks, vec_per_block;
};

// Frame t of the T+1 frame window of slot idx[j]: slots idx-T .. idx.  numpy wraps a negative window index to
// cap - T + (idx - T) (reference quirk for a valid slot below T, see oracle/replay_oracle.py gather()).
__device__ __forceinline__ const uint8_t* window_frame(const uint8_t* frames, const int64_t* idx, int j, int T, int64_t cap, int t,
                                                       size_t fbytes) {
  return frames + (size_t)window_slot(idx[j], T, cap, t) * fbytes;
}
// source frame of (which, cam, sample i, stack frame t): frame which + t of the T+1 window (train_utils.py:53-64: observation =
// frames 0..T-1, next observation = frames 1..T; T == 1: slot idx-1 and slot idx).
// Samples [0,count0) come from buffer 0, the rest from buffer 1.
__device__ __forceinline__ const uint8_t* source_frame(const GatherArgs& a, const StackJob& j, size_t fbytes) {
  if (a.from_packed) return a.packed[j.cam] + (size_t)stack_packed_frame(j, a.T) * fbytes;
  const int buf = (j.i < a.count0) ? 0 : 1;
  return window_frame(a.frames[buf][j.cam], a.idx[buf], buf == 0 ? j.i : j.i - a.count0, a.T, a.cap[buf], j.which + j.t, fbytes);
}
// (dy, dx) of frame i (= sample * T + stack frame); without a table it is the identity crop (4, 4)
__device__ __forceinline__ int2 crop_offset(const int32_t* crop, int i) {
  return make_int2(crop ? crop[2 * i] : 4, crop ? crop[2 * i + 1] : 4);
}
// frame workgroup -> (part of the frame, stack frame, sample, camera, which) (stack_index.h), with the source frame, the shift
// (sy, sx) and the frame's place in out_frames
struct FrameJob { int part, which, sy, sx; const uint8_t* src; size_t dst_frame; };
__device__ __forceinline__ FrameJob frame_job(const GatherArgs& a, int parts, size_t fbytes) {
  const StackJob s = stack_job((int)blockIdx.x, parts, a.T, a.batch, a.n_cam);
  FrameJob j;
  j.part = s.part; j.which = s.which;
  j.src = source_frame(a, s, fbytes);
  j.dst_frame = (size_t)stack_dst_frame(s, a.T, a.batch, a.n_cam);
  const int2 c = crop_offset(j.which == 0 ? a.crop_obs : a.crop_next, stack_crop_entry(s, a.T));
  j.sy = c.x - 4;
  j.sx = c.y - 4;
  return j;
}

// Shift one output row out of an LDS-staged source row.  rowb = W*C bytes (multiple of 16).
// Interior 16-byte chunks: 5 aligned dword LDS reads + v_alignbyte; edge chunks (where the shift
// clamps to the border pixel) are assembled per byte.
template <int CT>
__device__ __forceinline__ uint4 shifted_chunk(const uint8_t* srow, int q, int sx, int W, int Crt) {
  const int C = CT > 0 ? CT : Crt;  // compile-time channel count (3) turns the /C, %C below into shifts/mults
  const int o0 = q * 16;
  const int pmin = o0 / C, pmax = (o0 + 15) / C;
  uint4 r;
  if (pmin + sx >= 0 && pmax + sx <= W - 1) {
    const int b0 = o0 + sx * C;
    const uint32_t* w = reinterpret_cast<const uint32_t*>(srow + (b0 & ~3));
    const uint32_t sh = (uint32_t)(b0 & 3);
    uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
    r.x = __builtin_amdgcn_alignbyte(w1, w0, sh);
    r.y = __builtin_amdgcn_alignbyte(w2, w1, sh);
    r.z = __builtin_amdgcn_alignbyte(w3, w2, sh);
    r.w = __builtin_amdgcn_alignbyte(w4, w3, sh);
  } else {
    uint32_t words[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t v = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        int o = o0 + j * 4 + b;
        int p = o / C, ch = o - p * C;
        int sp = min(max(p + sx, 0), W - 1);
        v |= (uint32_t)srow[sp * C + ch] << (8 * b);
      }
      words[j] = v;
    }
    r = make_uint4(words[0], words[1], words[2], words[3]);
  }
  return r;
}

// the record of sample i
__device__ __forceinline__ const float* record_row(const GatherArgs& a, int i) {
  const int buf = (i < a.count0) ? 0 : 1;
  return a.rec[buf] + (size_t)a.idx[buf][buf == 0 ? i : i - a.count0] * a.rec_len;
}
__device__ __forceinline__ const float* record_row(const PackedArgs& a, int i) { return a.rec + (size_t)a.idx[i] * a.rec_len; }

// record gather: one thread per (sample, float of the record).  S = floats of a state; next states go to out_next_state
template <class Args>
__device__ __forceinline__ void gather_record(const Args& a, int e, int S, float* out_next_state) {
  const int i = e / a.rec_len, f = e - i * a.rec_len;
  if (i >= a.batch) return;
  const float v = record_row(a, i)[f];
  const int A = a.A;
  if (f < S) a.out_state[(size_t)i * S + f] = v;
  else if (f < 2 * S) out_next_state[(size_t)i * S + (f - S)] = v;
  else if (f < 2 * S + A) a.out_action[(size_t)i * A + (f - 2 * S)] = v;
  else if (f == 2 * S + A) a.out_reward[i] = v;
  else if (f == 2 * S + A + 1) a.out_mask[i] = v;
  else a.out_done[i] = (uint8_t)(v != 0.0f);
}

template <int CT>
__global__ __launch_bounds__(256) void gather_crop_kernel(GatherArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int tid = threadIdx.x;
  const int rowb = a.W * a.C;        // bytes per row
  const int lds_stride = rowb + 16;  // 16B pad: the 5th dword of the last chunk stays in bounds
  if ((int)blockIdx.x < a.n_frame_blocks) {
    const size_t fbytes = (size_t)a.H * rowb;
    const FrameJob j = frame_job(a, (a.H + kRowsPerBlock - 1) / kRowsPerBlock, fbytes);
    const int h0 = j.part * kRowsPerBlock;
    const int nrows = min(kRowsPerBlock, a.H - h0);
    const int vec_per_row = rowb / 16;
    // stage: LDS row r <- source row clamp(h0 + r + sy)
    for (int v = tid; v < nrows * vec_per_row; v += 256) {
      const int r = v / vec_per_row, q = v - r * vec_per_row;
      const int sh = min(max(h0 + r + j.sy, 0), a.H - 1);
      const uint4 val = *reinterpret_cast<const uint4*>(j.src + (size_t)sh * rowb + q * 16);
      *reinterpret_cast<uint4*>(lds + r * lds_stride + q * 16) = val;
    }
    __syncthreads();
    uint8_t* dst = a.out_frames + j.dst_frame * fbytes + (size_t)h0 * rowb;
    for (int v = tid; v < nrows * vec_per_row; v += 256) {
      const int r = v / vec_per_row, q = v - r * vec_per_row;
      const uint4 val = shifted_chunk<CT>(lds + r * lds_stride, q, j.sx, a.W, a.C);
      *reinterpret_cast<uint4*>(dst + (size_t)r * rowb + q * 16) = val;
    }
  } else if (!a.from_packed) {
    gather_record(a, (blockIdx.x - a.n_frame_blocks) * 256 + tid, a.S, a.out_state + (size_t)a.batch * a.S);
  }
}

// RGB frames (C == 3, W*3 a multiple of 16 and >= 32): no LDS.  Each output 16-byte vector is ONE unaligned 16-byte
// global load at byte offset q*16 + 3*sx of the (clamped) source row -- gfx950 global loads take any byte address --
// so a workgroup is a pure stream of independent load -> store pairs (4 vectors per thread, all loads in flight
// before the first store), with no barrier between a staging and a shifting phase.  Only the first / last vector of
// a row can reach past the row when sx != 0: its load is clamped into the row and the result is shifted by n = 3|sx|
// bytes with the border pixel replicated into the vacated bytes (n is a multiple of 3, so the replicated pattern's
// phase does not depend on n).  The arithmetic is uniform: no divergent edge path.
struct __attribute__((packed, aligned(1))) U128Unaligned { unsigned __int128 v; };
constexpr int kDirectVec = 4;  // vectors per thread

__global__ __launch_bounds__(256) void gather_crop_rgb_kernel(GatherArgs a) {
  const int tid = threadIdx.x;
  const int rowb = a.W * 3;
  const int vec_per_row = rowb >> 4;
  const int nvec = a.H * vec_per_row;
  if ((int)blockIdx.x < a.n_frame_blocks) {
    const size_t fbytes = (size_t)a.H * rowb;
    const FrameJob job = frame_job(a, (nvec + 256 * kDirectVec - 1) / (256 * kDirectVec), fbytes);
    const int part = job.part, sy = job.sy, sx3 = job.sx * 3;
    const uint8_t* src = job.src;
    uint8_t* dst = a.out_frames + job.dst_frame * fbytes;
    unsigned __int128 val[kDirectVec];
    int shl[kDirectVec], shr[kDirectVec];
#pragma unroll
    for (int j = 0; j < kDirectVec; ++j) {
      const int v = min((part * kDirectVec + j) * 256 + tid, nvec - 1);
      const int r = v / vec_per_row, q = v - r * vec_per_row;
      const int sh = min(max(r + sy, 0), a.H - 1);
      const int b0 = q * 16 + sx3;
      const int bc = min(max(b0, 0), rowb - 16);
      shl[j] = (bc - b0) * 8;   // > 0: left border, vector starts before the row
      shr[j] = (b0 - bc) * 8;   // > 0: right border
      val[j] = reinterpret_cast<const U128Unaligned*>(src + (size_t)sh * rowb + bc)->v;
    }
#pragma unroll
    for (int j = 0; j < kDirectVec; ++j) {
      const int v = (part * kDirectVec + j) * 256 + tid;
      unsigned __int128 x = val[j];
      const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 96);
      if (shl[j] > 0) {
        // bytes p0 p1 p2 of the first pixel; pattern byte k = p[k % 3]
        const uint32_t d0 = __builtin_amdgcn_perm(0, lo, 0x00020100u);  // p0 p1 p2 p0
        const uint32_t d1 = __builtin_amdgcn_perm(0, lo, 0x01000201u);  // p1 p2 p0 p1
        const uint32_t d2 = __builtin_amdgcn_perm(0, lo, 0x02010002u);  // p2 p0 p1 p2
        const unsigned __int128 pat = (unsigned __int128)d0 | ((unsigned __int128)d1 << 32) | ((unsigned __int128)d2 << 64) |
                                      ((unsigned __int128)d0 << 96);
        const unsigned __int128 keep = (~(unsigned __int128)0) << shl[j];
        x = (x << shl[j]) | (pat & ~keep);
      } else if (shr[j] > 0) {
        // bytes l0 l1 l2 of the last pixel = bytes 13..15 of the vector; pattern byte k = l[(k + 2) % 3]
        const uint32_t d0 = __builtin_amdgcn_perm(0, hi, 0x03020103u);  // l2 l0 l1 l2   (hi bytes: 1,2,3 = l0,l1,l2)
        const uint32_t d1 = __builtin_amdgcn_perm(0, hi, 0x01030201u);  // l0 l1 l2 l0
        const uint32_t d2 = __builtin_amdgcn_perm(0, hi, 0x02010302u);  // l1 l2 l0 l1
        const unsigned __int128 pat = (unsigned __int128)d0 | ((unsigned __int128)d1 << 32) | ((unsigned __int128)d2 << 64) |
                                      ((unsigned __int128)d0 << 96);
        const unsigned __int128 keep = (~(unsigned __int128)0) >> shr[j];
        x = (x >> shr[j]) | (pat & ~keep);
      }
      if (v < nvec) {
        uint4 o;
        o.x = (uint32_t)x; o.y = (uint32_t)(x >> 32); o.z = (uint32_t)(x >> 64); o.w = (uint32_t)(x >> 96);
        *reinterpret_cast<uint4*>(dst + (size_t)v * 16) = o;
      }
    }
  } else if (!a.from_packed) {
    gather_record(a, (blockIdx.x - a.n_frame_blocks) * 256 + tid, a.S, a.out_state + (size_t)a.batch * a.S);
  }
}

// sample(pack_obs_and_next_obs=True): straight 16B-vector copy of slots idx-T..idx per camera
__global__ __launch_bounds__(256) void gather_packed_kernel(PackedArgs a) {
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < a.n_frame_blocks) {
    const int blocks_per_frame = (int)((a.fbytes / 16 + a.vec_per_block - 1) / a.vec_per_block);
    int bid = blockIdx.x;
    const int part = bid % blocks_per_frame;
    bid /= blocks_per_frame;
    const int t = bid % (a.T + 1);
    bid /= (a.T + 1);
    const int i = bid % a.batch;
    const int cam = bid / a.batch;
    const uint4* src = reinterpret_cast<const uint4*>(window_frame(a.frames[cam], a.idx, i, a.T, a.cap, t, a.fbytes));
    uint4* dst = reinterpret_cast<uint4*>(a.out_frames[cam] + ((size_t)i * (a.T + 1) + t) * a.fbytes);
    const int nvec = (int)(a.fbytes / 16);
    const int v0 = part * a.vec_per_block;
    for (int v = v0 + tid; v < min(v0 + a.vec_per_block, nvec); v += 256) dst[v] = src[v];
  } else {
    gather_record(a, (blockIdx.x - a.n_frame_blocks) * 256 + tid, a.TS, a.out_next_state);
  }
}

// Batched insert: executes the op table of one launch (replay_batch.h), in no defined order.  A frame workgroup moves one
// (op, camera, 16 KB part) of frame bytes into the store, from the launch's staging entries or -- copy ops, the wrap re-insert --
// from another slot of the store; each thread issues its four 16-byte loads before its first store, as gather_crop_rgb_kernel
// does.  The workgroups after them move the records, one thread per (op, float).
struct ScatterArgs {
  uint8_t* frames[SERL_MAX_CAMS];
  float* rec;
  const uint8_t* entries;  // device copy of the launch's staging entries
  const BatchOp* ops;
  int n_ops, n_cam, parts, rec_len, n_frame_blocks;
  size_t fbytes, entry_bytes, rec_pad;
};

__global__ __launch_bounds__(256) void insert_scatter_kernel(ScatterArgs a) {
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < a.n_frame_blocks) {
    int bid = blockIdx.x;
    const int part = bid % a.parts;
    bid /= a.parts;
    const int cam = bid % a.n_cam;
    const BatchOp op = a.ops[bid / a.n_cam];
    const uint8_t* src = op.kind == SlotOp::kCopy ? a.frames[cam] + (size_t)op.src * a.fbytes
                                                  : a.entries + (size_t)op.src * a.entry_bytes + a.rec_pad + (size_t)cam * a.fbytes;
    uint8_t* dst = a.frames[cam] + (size_t)op.dst * a.fbytes;
    const int nvec = (int)(a.fbytes / 16);
    uint4 val[kDirectVec];
#pragma unroll
    for (int j = 0; j < kDirectVec; ++j) {
      const int v = min((part * kDirectVec + j) * 256 + tid, nvec - 1);
      val[j] = *reinterpret_cast<const uint4*>(src + (size_t)v * 16);
    }
#pragma unroll
    for (int j = 0; j < kDirectVec; ++j) {
      const int v = (part * kDirectVec + j) * 256 + tid;
      if (v < nvec) *reinterpret_cast<uint4*>(dst + (size_t)v * 16) = val[j];
    }
  } else {
    const int e = ((int)blockIdx.x - a.n_frame_blocks) * 256 + tid;
    const int o = e / a.rec_len, f = e - o * a.rec_len;
    if (o >= a.n_ops) return;
    const BatchOp op = a.ops[o];
    const float* src = op.kind == SlotOp::kCopy ? a.rec + (size_t)op.src * a.rec_len
                                                : reinterpret_cast<const float*>(a.entries + (size_t)op.src * a.entry_bytes);
    a.rec[(size_t)op.dst * a.rec_len + f] = src[f];
  }
}

// ---------------------------------------------------------------------------------------------
// host helpers
// ---------------------------------------------------------------------------------------------
// Declared in front of the lock of an index draw or a gather, so that it counts from before the wait for the mutex until after
// its release.
struct Reader {
  serl_rb* rbs[SERL_MAX_BUFFERS] = {nullptr};
  explicit Reader(serl_rb* a, serl_rb* b = nullptr) : rbs{a, b} {
    for (serl_rb* rb : rbs)
      if (rb) rb->readers.fetch_add(1);
  }
  ~Reader() {
    for (serl_rb* rb : rbs)
      if (rb) rb->readers.fetch_sub(1);
  }
  Reader(const Reader&) = delete;
  Reader& operator=(const Reader&) = delete;
};

// An insert must not overwrite a slot that an in-flight gather may still read: the copy stream waits (on the device)
// for the last enqueued gather.  Caller holds rb->mu.
static int order_after_gathers(serl_rb* rb) {
  if (rb->gather_pending) {
    for (int k = 0; k < serl_rb::kGatherStreams; ++k)
      if (rb->gather_pend[k]) {
        SERL_HIP(hipStreamWaitEvent(rb->copy_stream, rb->gather_ev[k], 0));
        rb->gather_pend[k] = false;
      }
    rb->gather_pending = false;
  }
  return SERL_OK;
}
// records "a gather of this buffer was enqueued on `stream`".  Caller holds rb->mu.
static int note_gather(serl_rb* rb, hipStream_t stream) {
  int k = -1;
  for (int i = 0; i < serl_rb::kGatherStreams && k < 0; ++i)
    if (rb->gather_used[i] && rb->gather_stream[i] == stream) k = i;
  if (k < 0) {   // a stream not seen before: take an entry with nothing pending, else recycle round-robin (the copy stream
                 // first waits for the recycled entry's gather, so nothing is forgotten)
    for (int i = 0; i < serl_rb::kGatherStreams && k < 0; ++i)
      if (!rb->gather_pend[i]) k = i;
    if (k < 0) {
      k = rb->gather_rr = (rb->gather_rr + 1) % serl_rb::kGatherStreams;
      SERL_HIP(hipStreamWaitEvent(rb->copy_stream, rb->gather_ev[k], 0));
    }
    rb->gather_stream[k] = stream;
    rb->gather_used[k] = true;
  }
  SERL_HIP(hipEventRecord(rb->gather_ev[k], stream));
  rb->gather_pend[k] = true;
  rb->gather_pending = true;
  return SERL_OK;
}
// ... and a gather enqueued after an insert sees it: `stream` waits for the last insert's copies.  Caller holds rb->mu.
// Once the last insert's event has COMPLETED the flag is cleared and later gathers carry no wait at all: until round 5 the flag
// was never cleared, so every gather -- the first command of every trunk pass -- opened with a cross-stream wait on a
// long-finished event (same-call A/B: pipelined 2.4497 / 2.4696 -> 2.4431 / 2.4544 ms, serial unchanged; NOT the cause of the
// 80-110 us of idle time at the pass boundary, profiles/README.md).
static int order_after_inserts(serl_rb* rb, hipStream_t stream) {
  if (!rb->insert_pending) return SERL_OK;
  const hipError_t q = hipEventQuery(rb->last_insert);
  if (q == hipSuccess) { rb->insert_pending = false; return SERL_OK; }
  if (q != hipErrorNotReady) SERL_HIP(q);
  (void)hipGetLastError();   // (hipErrorNotReady is sticky in hipGetLastError)
  SERL_HIP(hipStreamWaitEvent(stream, rb->last_insert, 0));
  return SERL_OK;
}

// writes slot `i` (record + one frame per camera) host -> HBM through the pinned ring.  Caller holds rb->mu.
static int write_slot(serl_rb* rb, int64_t i, const uint8_t* const* frames_host, const float* rec) {
  RC(rb->ins.acquire());
  uint8_t* h = rb->ins.h();
  const size_t rec_bytes = sizeof(float) * rb->rec_len;
  std::memcpy(h, rec, rec_bytes);
  const size_t f0 = rb->rec_pad;
  for (int c = 0; c < rb->n_cam; ++c) std::memcpy(h + f0 + (size_t)c * rb->frame_bytes, frames_host[c], rb->frame_bytes);
  SERL_HIP(hipMemcpyAsync(rb->rec + (size_t)i * rb->rec_len, h, rec_bytes, hipMemcpyHostToDevice, rb->copy_stream));
  for (int c = 0; c < rb->n_cam; ++c)
    SERL_HIP(hipMemcpyAsync(rb->frames[c] + (size_t)i * rb->frame_bytes, h + f0 + (size_t)c * rb->frame_bytes,
                            rb->frame_bytes, hipMemcpyHostToDevice, rb->copy_stream));
  rb->stats[2] += rb->n_cam + 1;
  return rb->ins.mark(rb->copy_stream);
}

// device->device copy of slot src to slot i (wrap re-insert, memory_efficient_replay_buffer.py:54-59).  Caller holds rb->mu.
static int copy_slot(serl_rb* rb, int64_t i, int64_t src) {
  SERL_HIP(hipMemcpyAsync(rb->rec + (size_t)i * rb->rec_len, rb->rec + (size_t)src * rb->rec_len,
                          sizeof(float) * rb->rec_len, hipMemcpyDeviceToDevice, rb->copy_stream));
  for (int c = 0; c < rb->n_cam; ++c)
    SERL_HIP(hipMemcpyAsync(rb->frames[c] + (size_t)i * rb->frame_bytes,
                            rb->frames[c] + (size_t)src * rb->frame_bytes, rb->frame_bytes,
                            hipMemcpyDeviceToDevice, rb->copy_stream));
  return SERL_OK;
}

// end of an insert: later gathers wait for its copies.  Caller holds rb->mu.
static int finish_insert(serl_rb* rb) {
  SERL_HIP(hipEventRecord(rb->last_insert, rb->copy_stream));
  rb->insert_pending = true;
  return SERL_OK;
}

// what both insert entry points check of their arguments: `n` transitions, frame tables of n * n_cam host pointers
static int check_insert_args(const serl_rb* rb, int64_t n, const uint8_t* const* obs_frames, const uint8_t* const* next_frames,
                             const float* state, const float* next_state, const float* action) {
  SERL_REQUIRE(rb && state && next_state && action, "NULL argument");
  SERL_REQUIRE(rb->n_cam == 0 || (obs_frames && next_frames), "NULL frames");
  for (int64_t k = 0; k < n * rb->n_cam; ++k)
    SERL_REQUIRE(obs_frames[k] && next_frames[k], "a frame pointer of transition %lld, camera %d is NULL", (long long)(k / rb->n_cam),
                 (int)(k % rb->n_cam));
  return SERL_OK;
}
// the record of a transition: [state T*S | next_state T*S | action A | reward | mask | done]
static void pack_record(const serl_rb* rb, float* rec, const float* state, const float* next_state, const float* action, float reward,
                        float mask, bool done) {
  const int TS = rb->T * rb->S;
  std::memcpy(rec, state, sizeof(float) * TS);
  std::memcpy(rec + TS, next_state, sizeof(float) * TS);
  std::memcpy(rec + 2 * TS, action, sizeof(float) * rb->A);
  rec[2 * TS + rb->A] = reward;
  rec[2 * TS + rb->A + 1] = mask;
  rec[2 * TS + rb->A + 2] = done ? 1.0f : 0.0f;
}

// ---- batched insert.  The caller holds rb->mu throughout.
// The staging ring of the launches, made at the first batched call: a slot holds as many entries as fit kBatBudget with their
// places in the op table (at least one), and the table's places for the copies of a wrap.
static int batch_init(serl_rb* rb) {
  if (rb->bat.n) return SERL_OK;
  const size_t per_entry = rb->entry_bytes + sizeof(BatchOp), fixed = sizeof(BatchOp) * (size_t)rb->T;
  const size_t entries = std::min<size_t>(std::max<size_t>((kBatBudget - std::min(fixed, kBatBudget)) / per_entry, 1), 1 << 20);
  rb->plan.init(rb->ix.cap, rb->T, (int)entries);
  const int rc = rb->bat.init(kBatRing, entries * rb->entry_bytes + sizeof(BatchOp) * (size_t)rb->plan.max_ops, true);
  if (rc != SERL_OK) {  // nothing half-built stays behind: the next call tries again
    rb->bat.destroy();
    rb->bat = StageRing();
  }
  return rc;
}
// the launch being built gets its staging slot when it first needs one
static int take_batch_slot(serl_rb* rb) {
  if (!rb->bat_taken) RC(rb->bat.acquire());
  rb->bat_taken = true;
  return SERL_OK;
}
struct BatchSource {  // the arguments of serl_rb_insert_batch
  const uint8_t* const* obs_frames;
  const uint8_t* const* next_frames;
  const float *state, *next_state, *action, *reward, *mask;
  const uint8_t* done;
};
// fills the staging entry of write op `op` from its transition
static int fill_entry(serl_rb* rb, const BatchOp& op, const BatchSource& in) {
  RC(take_batch_slot(rb));
  uint8_t* e = rb->bat.h() + (size_t)op.src * rb->entry_bytes;
  const size_t tr = (size_t)op.tr, TS = (size_t)rb->T * rb->S;
  pack_record(rb, reinterpret_cast<float*>(e), in.state + tr * TS, in.next_state + tr * TS, in.action + tr * rb->A, in.reward[tr],
              in.mask[tr], in.done[tr] != 0);
  const uint8_t* const* from = (op.kind == SlotOp::kObsFrame ? in.obs_frames : in.next_frames) + tr * rb->n_cam;
  for (int c = 0; c < rb->n_cam; ++c)
    std::memcpy(e + rb->rec_pad + (size_t)c * rb->frame_bytes, from[c] + (size_t)op.frame * rb->frame_bytes, rb->frame_bytes);
  return SERL_OK;
}
// runs the launch built in rb->plan: ONE H2D copy of its entries and its op table (which lies behind the last entry used), ONE
// kernel
static int run_launch(serl_rb* rb) {
  const BatchPlan& p = rb->plan;
  RC(take_batch_slot(rb));  // (a launch of copies only has no entry)
  const size_t table_at = (size_t)p.entries * rb->entry_bytes, table_bytes = sizeof(BatchOp) * p.ops.size();
  std::memcpy(rb->bat.h() + table_at, p.ops.data(), table_bytes);
  SERL_HIP(hipMemcpyAsync(rb->bat.d(), rb->bat.h(), table_at + table_bytes, hipMemcpyHostToDevice, rb->copy_stream));
  ScatterArgs a{};
  for (int c = 0; c < rb->n_cam; ++c) a.frames[c] = rb->frames[c];
  a.rec = rb->rec;
  a.entries = rb->bat.d();
  a.ops = reinterpret_cast<const BatchOp*>(rb->bat.d() + table_at);
  a.n_ops = (int)p.ops.size(); a.n_cam = rb->n_cam; a.rec_len = rb->rec_len;
  a.fbytes = rb->frame_bytes; a.entry_bytes = rb->entry_bytes; a.rec_pad = rb->rec_pad;
  a.parts = cdiv((long)(rb->frame_bytes / 16), 256 * kDirectVec);
  const int64_t frame_blocks = (int64_t)a.n_ops * rb->n_cam * a.parts, rec_blocks = cdiv((long)a.n_ops * rb->rec_len, 256);
  SERL_REQUIRE(frame_blocks + rec_blocks < (1LL << 31), "a launch of %d slot operations needs too many workgroups", a.n_ops);
  a.n_frame_blocks = (int)frame_blocks;
  hipLaunchKernelGGL(insert_scatter_kernel, dim3((unsigned)(frame_blocks + rec_blocks)), dim3(256), 0, rb->copy_stream, a);
  SERL_HIP(hipGetLastError());
  rb->bat_taken = false;
  rb->stats[2] += 1;
  rb->stats[3] += 1;
  return rb->bat.mark(rb->copy_stream);
}

// lays `n` host sources out at 16-byte alignment in a slot of `ring` (a NULL source keeps its place and is not copied) and
// enqueues ONE H2D copy of the slot on `stream`; *dev_out is the slot's device address, offsets[k] where source k lies in it.
// A total beyond the slot is refused before a slot is taken or a byte copied.  The caller launches, then ring.mark(stream).
static int stage_params(StageRing& ring, const void* const* srcs, const size_t* sizes, int n,
                        hipStream_t stream, uint8_t** dev_out, size_t* offsets) {
  size_t total = 0;
  for (int k = 0; k < n; ++k) {
    offsets[k] = total;
    total += (sizes[k] + 15) & ~(size_t)15;
  }
  SERL_REQUIRE(total <= ring.slot_bytes, "batch too large for the staging slot (%zu > %zu bytes)", total, ring.slot_bytes);
  RC(ring.acquire());
  for (int k = 0; k < n; ++k)
    if (srcs[k]) std::memcpy(ring.h() + offsets[k], srcs[k], sizes[k]);
  // (round 5: letting the gather kernel read the pinned host slot itself -- no copy command on the stream -- left the step
  //  unchanged, 2.5225 / 2.5198 -> 2.5221 / 2.5239 ms: the idle time in front of a pass is not the copy's, profiles/README.md)
  SERL_HIP(hipMemcpyAsync(ring.d(), ring.h(), total, hipMemcpyHostToDevice, stream));
  *dev_out = ring.d();
  return SERL_OK;
}

// what a gather checks of its indices: in range, and stale ones re-drawn in place (ReplayIndex::revalidate).  Caller holds rb->mu.
static int check_and_revalidate(serl_rb* rb, int64_t* idx, int n) {
  int bad = 0;
  if (rb->ix.check_indices(idx, n, &bad) != IndexStatus::kOk) {
    set_error("index %lld out of range [0,%lld)", (long long)idx[bad], (long long)rb->ix.size);
    return SERL_ERR_INVALID;
  }
  const IndexStatus st = rb->ix.revalidate(idx, n);
  SERL_REQUIRE(st != IndexStatus::kNotSeeded, "replay buffer RNG not seeded");
  SERL_REQUIRE(st != IndexStatus::kRedrawExhausted, "no valid slot found while re-drawing a stale index");
  return SERL_OK;
}

// ---------------------------------------------------------------------------------------------
// snapshot export / import: HBM <-> ordinary host memory in chunks through two pinned buffers on the copy stream
// ---------------------------------------------------------------------------------------------
static int xfer_init(serl_rb* rb) {
  if (!rb->xfer_host) SERL_HIP(hipHostMalloc((void**)&rb->xfer_host, 2 * kXferChunk, hipHostMallocDefault));
  for (int k = 0; k < 2; ++k)
    if (!rb->xfer_done[k]) SERL_HIP(hipEventCreateWithFlags(&rb->xfer_done[k], hipEventDisableTiming));
  return SERL_OK;
}
// Chunk i goes through buffer i & 1; chunk i + 1 is in flight while chunk i is copied out of its buffer.
static int staged_d2h(serl_rb* rb, uint8_t* dst, const uint8_t* dev_src, size_t bytes) {
  const size_t n = (bytes + kXferChunk - 1) / kXferChunk;
  for (size_t i = 0; i <= n; ++i) {
    if (i < n) {
      const size_t off = i * kXferChunk, len = bytes - off < kXferChunk ? bytes - off : kXferChunk;
      SERL_HIP(hipMemcpyAsync(rb->xfer_host + (i & 1) * kXferChunk, dev_src + off, len, hipMemcpyDeviceToHost, rb->copy_stream));
      SERL_HIP(hipEventRecord(rb->xfer_done[i & 1], rb->copy_stream));
    }
    if (i >= 1) {
      const size_t off = (i - 1) * kXferChunk, len = bytes - off < kXferChunk ? bytes - off : kXferChunk;
      SERL_HIP(hipEventSynchronize(rb->xfer_done[(i - 1) & 1]));
      std::memcpy(dst + off, rb->xfer_host + ((i - 1) & 1) * kXferChunk, len);
    }
  }
  return SERL_OK;
}
// A buffer is refilled once the copy that last read it has completed (an event never recorded counts as complete); the caller
// synchronises the copy stream at the end.
static int staged_h2d(serl_rb* rb, uint8_t* dev_dst, const uint8_t* src, size_t bytes) {
  const size_t n = (bytes + kXferChunk - 1) / kXferChunk;
  for (size_t i = 0; i < n; ++i) {
    const size_t off = i * kXferChunk, len = bytes - off < kXferChunk ? bytes - off : kXferChunk;
    uint8_t* h = rb->xfer_host + (i & 1) * kXferChunk;
    SERL_HIP(hipEventSynchronize(rb->xfer_done[i & 1]));
    std::memcpy(h, src + off, len);
    SERL_HIP(hipMemcpyAsync(dev_dst + off, h, len, hipMemcpyHostToDevice, rb->copy_stream));
    SERL_HIP(hipEventRecord(rb->xfer_done[i & 1], rb->copy_stream));
  }
  return SERL_OK;
}
static int check_slot_range(const serl_rb* rb, int64_t slot_begin, int64_t n_slots, const uint8_t* const* frames, const void* records) {
  SERL_REQUIRE(slot_begin >= 0 && slot_begin < rb->ix.cap, "slot_begin %lld not in [0,%lld)", (long long)slot_begin, (long long)rb->ix.cap);
  SERL_REQUIRE(n_slots >= 0 && n_slots <= rb->ix.cap, "n_slots %lld not in [0,%lld]", (long long)n_slots, (long long)rb->ix.cap);
  if (n_slots == 0) return SERL_OK;
  SERL_REQUIRE(records && (rb->n_cam == 0 || frames), "NULL argument");
  for (int c = 0; c < rb->n_cam; ++c) SERL_REQUIRE(frames[c], "frames[%d] is NULL", c);
  return SERL_OK;
}
// the device reads of an export; the store is marked busy, the mutex is NOT held
static int export_copies(serl_rb* rb, int64_t slot_begin, int64_t n_slots, uint8_t* const* host_frames, float* host_records) {
  SERL_HIP(hipSetDevice(rb->device));
  SERL_HIP(hipEventSynchronize(rb->last_insert));  // the copies of the last insert (the copy stream orders the reads behind them too)
  SlotRun runs[2];
  const int nr = rb->ix.slot_runs(slot_begin, n_slots, runs);
  const size_t rec_bytes = sizeof(float) * rb->rec_len;
  for (int r = 0; r < nr; ++r) {
    RC(staged_d2h(rb, reinterpret_cast<uint8_t*>(host_records) + (size_t)runs[r].at * rec_bytes,
                  reinterpret_cast<const uint8_t*>(rb->rec) + (size_t)runs[r].slot * rec_bytes, (size_t)runs[r].n * rec_bytes));
    for (int c = 0; c < rb->n_cam; ++c)
      RC(staged_d2h(rb, host_frames[c] + (size_t)runs[r].at * rb->frame_bytes, rb->frames[c] + (size_t)runs[r].slot * rb->frame_bytes,
                    (size_t)runs[r].n * rb->frame_bytes));
  }
  return SERL_OK;
}

}  // namespace serl

using namespace serl;

extern "C" {

const char* serl_last_error(void) { return serl::g_err; }
int serl_version(void) { return 100; }
int serl_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int serl_rb_create(int device, int64_t capacity, int n_cam, int H, int W, int C, int num_stack,
                   int state_dim, int act_dim, serl_rb** out) {
  SERL_REQUIRE(out != nullptr, "out is NULL");
  SERL_REQUIRE(capacity > 1 && capacity < 0x7FFFFFFF, "capacity %lld out of range", (long long)capacity);
  // n_cam == 0: plain ReplayBuffer of flat observations (replay_buffer.py:41-75): every inserted slot is valid
  SERL_REQUIRE(n_cam >= 0 && n_cam <= SERL_MAX_CAMS, "n_cam %d not in [0,%d]", n_cam, SERL_MAX_CAMS);
  SERL_REQUIRE(num_stack >= 1, "num_stack must be >= 1");
  if (n_cam == 0) { H = W = C = 0; }
  SERL_REQUIRE(n_cam == 0 || ((size_t)W * C) % 16 == 0, "W*C (%d) must be a multiple of 16 bytes", W * C);
  SERL_REQUIRE((n_cam == 0 || H >= 1) && state_dim >= 1 && act_dim >= 1, "bad dims");
  SERL_HIP(hipSetDevice(device));
  // one owner until the end: every failure below frees what was built (serl_rb_destroy tolerates a half-built store)
  std::unique_ptr<serl_rb, int (*)(serl_rb*)> rb(new serl_rb(), serl_rb_destroy);
  rb->device = device;
  rb->n_cam = n_cam;
  rb->H = H; rb->W = W; rb->C = C; rb->T = num_stack; rb->S = state_dim; rb->A = act_dim;
  rb->rec_len = 2 * num_stack * state_dim + act_dim + 3;
  rb->frame_bytes = (size_t)H * W * C;
  rb->rec_pad = (sizeof(float) * rb->rec_len + 255) & ~(size_t)255;
  rb->entry_bytes = rb->rec_pad + (size_t)n_cam * rb->frame_bytes;
  rb->ix.init(capacity, n_cam > 0, num_stack);
  for (int c = 0; c < n_cam; ++c) {
    hipError_t e = hipMalloc((void**)&rb->frames[c], (size_t)capacity * rb->frame_bytes);
    if (e != hipSuccess) {
      set_error("hipMalloc of %zu bytes for camera %d failed: %s", (size_t)capacity * rb->frame_bytes,
                c, hipGetErrorString(e));
      return SERL_ERR_HIP;
    }
  }
  SERL_HIP(hipMalloc((void**)&rb->rec, (size_t)capacity * rb->rec_len * sizeof(float)));
  SERL_HIP(hipStreamCreateWithFlags(&rb->copy_stream, hipStreamNonBlocking));
  for (int k = 0; k < serl_rb::kGatherStreams; ++k) SERL_HIP(hipEventCreateWithFlags(&rb->gather_ev[k], hipEventDisableTiming));
  SERL_HIP(hipEventCreateWithFlags(&rb->last_insert, hipEventDisableTiming));
  RC(rb->ins.init(kInsRing, rb->entry_bytes, false));
  RC(rb->stage.init(kRing, (size_t)(1 << 16) * std::min(num_stack, kMaxStack), true));  // idx (8B) + 2 crops (16B per frame) per sample: up to ~2700 samples
  *out = rb.release();
  return SERL_OK;
}

int serl_rb_destroy(serl_rb* rb) {
  if (!rb) return SERL_OK;
  (void)hipSetDevice(rb->device);
  if (rb->copy_stream) (void)hipStreamSynchronize(rb->copy_stream);
  for (int c = 0; c < SERL_MAX_CAMS; ++c)
    if (rb->frames[c]) (void)hipFree(rb->frames[c]);
  if (rb->rec) (void)hipFree(rb->rec);
  rb->stage.destroy();
  for (int k = 0; k < serl_rb::kGatherStreams; ++k)
    if (rb->gather_ev[k]) (void)hipEventDestroy(rb->gather_ev[k]);
  if (rb->last_insert) (void)hipEventDestroy(rb->last_insert);
  rb->ins.destroy();
  rb->bat.destroy();
  if (rb->xfer_host) (void)hipHostFree(rb->xfer_host);
  for (int k = 0; k < 2; ++k)
    if (rb->xfer_done[k]) (void)hipEventDestroy(rb->xfer_done[k]);
  if (rb->copy_stream) (void)hipStreamDestroy(rb->copy_stream);
  delete rb;
  return SERL_OK;
}

int serl_rb_seed(serl_rb* rb, uint64_t state_hi, uint64_t state_lo, uint64_t inc_hi,
                 uint64_t inc_lo, int has_uint32, uint32_t uinteger) {
  SERL_REQUIRE(rb, "rb is NULL");
  std::lock_guard<std::mutex> g(rb->mu);
  const uint64_t words[4] = {state_hi, state_lo, inc_hi, inc_lo};
  rb->ix.rng.set(words, has_uint32, uinteger);
  return SERL_OK;
}

int serl_rb_rng_state(serl_rb* rb, uint64_t out[4], int* has_uint32, uint32_t* uinteger) {
  SERL_REQUIRE(rb && out && has_uint32 && uinteger, "NULL argument");
  std::lock_guard<std::mutex> g(rb->mu);
  rb->ix.rng.get(out);
  *has_uint32 = rb->ix.rng.has_uint32;
  *uinteger = rb->ix.rng.uinteger;
  return SERL_OK;
}

int serl_rb_insert(serl_rb* rb, const uint8_t* const* obs_frames, const uint8_t* const* next_frames,
                   const float* state, const float* next_state, const float* action, float reward,
                   float mask, int done) {
  RC(check_insert_args(rb, 1, obs_frames, next_frames, state, next_state, action));
  std::unique_lock<std::mutex> g(rb->mu);
  rb->idle.wait(g, [rb] { return !rb->busy; });  // a snapshot export is reading the slots
  SERL_HIP(hipSetDevice(rb->device));
  RC(order_after_gathers(rb));  // never overwrite a slot an in-flight gather may still read
  std::vector<float> rec(rb->rec_len);
  pack_record(rb, rec.data(), state, next_state, action, reward, mask, done != 0);
  rb->stats[0] += 1;
  const uint8_t* fr[SERL_MAX_CAMS];
  for (const SlotOp& op : rb->ix.plan_insert(done != 0)) {
    if (op.kind == SlotOp::kCopy) {
      RC(copy_slot(rb, op.dst, op.arg));
    } else {
      const uint8_t* const* from = op.kind == SlotOp::kObsFrame ? obs_frames : next_frames;
      for (int c = 0; c < rb->n_cam; ++c) fr[c] = from[c] + (size_t)op.arg * rb->frame_bytes;
      RC(write_slot(rb, op.dst, fr, rec.data()));
    }
  }
  return finish_insert(rb);
}

// The transitions go in under the mutex in groups: a group is as many whole transitions as one staging slot is sure to hold
// (a launch is also cut wherever replay_batch.h says so, inside a transition if need be, with the mutex kept).  Per group: wait
// for a snapshot export to end, order the copy stream behind the gathers in flight, plan, fill the pinned slot, enqueue, record
// last_insert.  The mutex is released between groups only, so every transition is wholly in a snapshot export or not in it, and
// never across a stream synchronisation other than StageRing::acquire waiting for its own slot of two launches ago.
int serl_rb_insert_batch(serl_rb* rb, int n, const uint8_t* const* obs_frames, const uint8_t* const* next_frames, const float* state,
                         const float* next_state, const float* action, const float* reward, const float* mask, const uint8_t* done) {
  SERL_REQUIRE(rb, "rb is NULL");
  SERL_REQUIRE(n >= 0, "negative transition count %d", n);
  if (n == 0) return SERL_OK;
  RC(check_insert_args(rb, n, obs_frames, next_frames, state, next_state, action));
  SERL_REQUIRE(reward && mask && done, "NULL argument");
  const BatchSource in{obs_frames, next_frames, state, next_state, action, reward, mask, done};
  std::unique_lock<std::mutex> g(rb->mu);
  SERL_HIP(hipSetDevice(rb->device));
  RC(batch_init(rb));
  rb->plan.clear();  // (a call that failed half way may have left a launch behind)
  rb->bat_taken = false;
  rb->stats[1] += 1;
  bool group_open = false;
  for (int i = 0; i < n; ++i) {
    if (!group_open) {
      rb->idle.wait(g, [rb] { return !rb->busy; });  // a snapshot export is reading the slots
      RC(order_after_gathers(rb));                    // never overwrite a slot an in-flight gather may still read
      group_open = true;
    }
    for (const SlotOp& op : rb->ix.plan_insert(done[i] != 0)) {
      RC(rb->plan.push(op, i, [rb] { return run_launch(rb); }));
      if (op.kind != SlotOp::kCopy) RC(fill_entry(rb, rb->plan.ops.back(), in));
    }
    rb->stats[0] += 1;
    if (i + 1 == n || !rb->plan.room_for_transition()) {
      RC(run_launch(rb));
      rb->plan.clear();
      RC(finish_insert(rb));
      if (i + 1 < n) {  // let the index draws and gathers that wait for the mutex in
        g.unlock();
        const auto give_up = std::chrono::steady_clock::now() + std::chrono::microseconds(kHandOverUs);
        while (rb->readers.load(std::memory_order_relaxed) > 0 && std::chrono::steady_clock::now() < give_up) std::this_thread::yield();
        g.lock();
        group_open = false;
      }
    }
  }
  return SERL_OK;
}

int serl_rb_insert_stats(serl_rb* rb, int64_t out[4]) {
  SERL_REQUIRE(rb && out, "NULL argument");
  std::lock_guard<std::mutex> g(rb->mu);
  std::memcpy(out, rb->stats, sizeof(rb->stats));
  return SERL_OK;
}

int64_t serl_rb_len(serl_rb* rb) {
  if (!rb) return -1;
  std::lock_guard<std::mutex> g(rb->mu);
  return rb->ix.size;
}
int64_t serl_rb_insert_index(serl_rb* rb) {
  if (!rb) return -1;
  std::lock_guard<std::mutex> g(rb->mu);
  return rb->ix.insert_index;
}
int64_t serl_rb_insert_count(serl_rb* rb) {
  if (!rb) return -1;
  std::lock_guard<std::mutex> g(rb->mu);
  return rb->ix.insert_count;
}
int serl_rb_valid_mask(serl_rb* rb, uint8_t* host_out) {
  SERL_REQUIRE(rb && host_out, "NULL argument");
  std::lock_guard<std::mutex> g(rb->mu);
  std::memcpy(host_out, rb->ix.valid.data(), (size_t)rb->ix.cap);
  return SERL_OK;
}

int serl_rb_export_meta(serl_rb* rb, serl_rb_meta* out) {
  SERL_REQUIRE(rb && out, "NULL argument");
  std::lock_guard<std::mutex> g(rb->mu);
  std::memset(out, 0, sizeof(*out));
  out->capacity = rb->ix.cap;
  out->n_cam = rb->n_cam; out->H = rb->H; out->W = rb->W; out->C = rb->C; out->T = rb->T; out->S = rb->S; out->A = rb->A;
  out->rec_len = rb->rec_len;
  out->size = rb->ix.size; out->insert_index = rb->ix.insert_index; out->insert_count = rb->ix.insert_count;
  out->first = rb->ix.first ? 1 : 0;
  out->rng_seeded = rb->ix.rng.seeded ? 1 : 0;
  rb->ix.rng.get(out->rng_state_inc);
  out->rng_has_uint32 = rb->ix.rng.has_uint32;
  out->rng_uinteger = rb->ix.rng.uinteger;
  return SERL_OK;
}

int serl_rb_export_slots(serl_rb* rb, int64_t slot_begin, int64_t n_slots, uint8_t* const* host_frames, float* host_records,
                         uint8_t* host_valid) {
  SERL_REQUIRE(rb, "rb is NULL");
  RC(check_slot_range(rb, slot_begin, n_slots, host_frames, host_records));
  {
    std::unique_lock<std::mutex> g(rb->mu);
    rb->idle.wait(g, [rb] { return !rb->busy; });
    SERL_HIP(hipSetDevice(rb->device));
    RC(xfer_init(rb));
    // the mask belongs to the same instant as the slots: no insert runs between here and the end of the copies
    if (host_valid) std::memcpy(host_valid, rb->ix.valid.data(), (size_t)rb->ix.cap);
    rb->busy = true;
  }
  // mutex released: sample_indices and gathers go on; inserts wait on `idle`
  const int rc = export_copies(rb, slot_begin, n_slots, host_frames, host_records);
  {
    std::lock_guard<std::mutex> g(rb->mu);
    rb->busy = false;
  }
  rb->idle.notify_all();
  return rc;
}

int serl_rb_import_meta(serl_rb* rb, const serl_rb_meta* m) {
  SERL_REQUIRE(rb && m, "NULL argument");
  std::unique_lock<std::mutex> g(rb->mu);
  rb->idle.wait(g, [rb] { return !rb->busy; });
  SERL_REQUIRE(m->capacity == rb->ix.cap && m->n_cam == rb->n_cam && m->H == rb->H && m->W == rb->W && m->C == rb->C && m->T == rb->T &&
                   m->S == rb->S && m->A == rb->A && m->rec_len == rb->rec_len,
               "snapshot geometry (capacity %lld, %d cameras %dx%dx%d, T %d, S %d, A %d) is not the store's (capacity %lld, %d cameras "
               "%dx%dx%d, T %d, S %d, A %d)", (long long)m->capacity, m->n_cam, m->H, m->W, m->C, m->T, m->S, m->A, (long long)rb->ix.cap,
               rb->n_cam, rb->H, rb->W, rb->C, rb->T, rb->S, rb->A);
  SERL_REQUIRE(rb->ix.restore(m->size, m->insert_index, m->insert_count, m->first != 0) == IndexStatus::kOk,
               "inconsistent bookkeeping: size %lld, insert_index %lld, insert_count %lld at capacity %lld", (long long)m->size,
               (long long)m->insert_index, (long long)m->insert_count, (long long)rb->ix.cap);
  if (m->rng_seeded) rb->ix.rng.set(m->rng_state_inc, m->rng_has_uint32, m->rng_uinteger);
  return SERL_OK;
}

int serl_rb_import_slots(serl_rb* rb, int64_t slot_begin, int64_t n_slots, const uint8_t* const* host_frames,
                         const float* host_records, const uint8_t* host_valid) {
  SERL_REQUIRE(rb, "rb is NULL");
  RC(check_slot_range(rb, slot_begin, n_slots, host_frames, host_records));
  std::unique_lock<std::mutex> g(rb->mu);
  rb->idle.wait(g, [rb] { return !rb->busy; });
  SERL_HIP(hipSetDevice(rb->device));
  RC(xfer_init(rb));
  RC(order_after_gathers(rb));  // as an insert: never overwrite a slot an in-flight gather may still read
  SlotRun runs[2];
  const int nr = rb->ix.slot_runs(slot_begin, n_slots, runs);
  const size_t rec_bytes = sizeof(float) * rb->rec_len;
  for (int r = 0; r < nr; ++r) {
    const uint8_t* rec_src = reinterpret_cast<const uint8_t*>(host_records) + (size_t)runs[r].at * rec_bytes;
    RC(staged_h2d(rb, reinterpret_cast<uint8_t*>(rb->rec) + (size_t)runs[r].slot * rec_bytes, rec_src, (size_t)runs[r].n * rec_bytes));
    for (int c = 0; c < rb->n_cam; ++c)
      RC(staged_h2d(rb, rb->frames[c] + (size_t)runs[r].slot * rb->frame_bytes, host_frames[c] + (size_t)runs[r].at * rb->frame_bytes,
                    (size_t)runs[r].n * rb->frame_bytes));
  }
  if (host_valid) std::memcpy(rb->ix.valid.data(), host_valid, (size_t)rb->ix.cap);
  SERL_HIP(hipStreamSynchronize(rb->copy_stream));  // the slots are in HBM when the call returns: a later gather needs no wait
  return SERL_OK;
}

int serl_rb_sample_indices(serl_rb* rb, int batch, int64_t* host_idx_out) {
  SERL_REQUIRE(rb && host_idx_out, "NULL argument");
  SERL_REQUIRE(batch >= 0, "negative batch");
  Reader reader(rb);
  std::lock_guard<std::mutex> g(rb->mu);
  const IndexStatus st = rb->ix.sample(batch, host_idx_out);
  if (st == IndexStatus::kOk) return SERL_OK;
  set_error("%s", st == IndexStatus::kNotSeeded ? "replay buffer RNG not seeded: call serl_rb_seed first"
                  : st == IndexStatus::kEmpty   ? "cannot sample from an empty replay buffer"
                                                : "replay buffer holds no valid transition");
  return SERL_ERR_STATE;
}

int serl_rb_gather_packed(serl_rb* rb, int64_t* host_idx, int batch,
                          uint8_t* const* dev_frames_out, float* dev_state_out,
                          float* dev_next_state_out, float* dev_action_out, float* dev_reward_out,
                          float* dev_mask_out, uint8_t* dev_done_out, void* stream_) {
  SERL_REQUIRE(rb && host_idx && (dev_frames_out || rb->n_cam == 0), "NULL argument");
  SERL_REQUIRE(batch > 0, "batch must be positive");
  hipStream_t stream = (hipStream_t)stream_;
  Reader reader(rb);
  std::lock_guard<std::mutex> g(rb->mu);
  SERL_HIP(hipSetDevice(rb->device));
  RC(check_and_revalidate(rb, host_idx, batch));
  RC(order_after_inserts(rb, stream));
  const void* srcs[1] = {host_idx};
  size_t sizes[1] = {sizeof(int64_t) * (size_t)batch}, offs[1];
  uint8_t* dparams;
  RC(stage_params(rb->stage, srcs, sizes, 1, stream, &dparams, offs));
  PackedArgs a{};
  for (int c = 0; c < rb->n_cam; ++c) {
    a.frames[c] = rb->frames[c];
    a.out_frames[c] = dev_frames_out[c];
  }
  a.rec = rb->rec;
  a.idx = reinterpret_cast<const int64_t*>(dparams + offs[0]);
  a.batch = batch; a.n_cam = rb->n_cam; a.T = rb->T; a.TS = rb->T * rb->S; a.A = rb->A;
  a.rec_len = rb->rec_len; a.fbytes = rb->frame_bytes; a.cap = rb->ix.cap;
  a.out_state = dev_state_out; a.out_next_state = dev_next_state_out; a.out_action = dev_action_out;
  a.out_reward = dev_reward_out; a.out_mask = dev_mask_out; a.out_done = dev_done_out;
  a.vec_per_block = 256 * 4;
  const int blocks_per_frame = cdiv((long)(rb->frame_bytes / 16), a.vec_per_block);
  a.n_frame_blocks = rb->n_cam * batch * (rb->T + 1) * blocks_per_frame;
  const int rec_blocks = dev_state_out ? cdiv((long)batch * rb->rec_len, 256) : 0;
  hipLaunchKernelGGL(gather_packed_kernel, dim3(a.n_frame_blocks + rec_blocks), dim3(256), 0, stream, a);
  SERL_HIP(hipGetLastError());
  RC(rb->stage.mark(stream));
  return note_gather(rb, stream);
}

// a table of (dy, dx) per frame, or none
static int check_crops(const int32_t* crop, int batch) {
  if (crop)
    for (int i = 0; i < 2 * batch; ++i) SERL_REQUIRE(crop[i] >= 0 && crop[i] <= 8, "crop offset %d out of [0,8]", crop[i]);
  return SERL_OK;
}

static int set_frame_blocks(GatherArgs& a, int parts) {
  const int64_t n = stack_frame_blocks(parts, a.T, a.batch, a.n_cam);
  SERL_REQUIRE(n + cdiv((long)a.batch * a.rec_len, 256) < (1LL << 31), "gather+crop of %d x %d frames needs too many workgroups", a.batch, a.T);
  a.n_frame_blocks = (int)n;
  return SERL_OK;
}

static int launch_gather_crop(GatherArgs& a, hipStream_t stream) {
  const int rec_blocks = a.from_packed ? 0 : cdiv((long)a.batch * a.rec_len, 256);
  ProfScope prof("gather_crop", stream);
  if (a.C == 3 && (a.W * 3) % 16 == 0 && a.W * 3 >= 32) {   // RGB rows of whole 16-byte vectors: the LDS-free kernel
    const int nvec = a.H * (a.W * 3 / 16);
    RC(set_frame_blocks(a, cdiv(nvec, 256 * kDirectVec)));
    hipLaunchKernelGGL(gather_crop_rgb_kernel, dim3(a.n_frame_blocks + rec_blocks), dim3(256), 0, stream, a);
    SERL_HIP(hipGetLastError());
    return SERL_OK;
  }
  const int chunks = cdiv(a.H, kRowsPerBlock);
  RC(set_frame_blocks(a, chunks));
  const size_t lds = (size_t)kRowsPerBlock * ((size_t)a.W * a.C + 16);
  if (a.C == 3) hipLaunchKernelGGL(gather_crop_kernel<3>, dim3(a.n_frame_blocks + rec_blocks), dim3(256), lds, stream, a);
  else hipLaunchKernelGGL(gather_crop_kernel<0>, dim3(a.n_frame_blocks + rec_blocks), dim3(256), lds, stream, a);
  SERL_HIP(hipGetLastError());
  return SERL_OK;
}

int serl_rb_gather_crop(serl_rb* const* rbs, int n_rb, int64_t* const* host_idx,
                        const int* counts, const int32_t* host_crop_obs,
                        const int32_t* host_crop_next, const serl_batch* out, void* stream_) {
  SERL_REQUIRE(rbs && host_idx && counts && out, "NULL argument");
  SERL_REQUIRE(n_rb >= 1 && n_rb <= SERL_MAX_BUFFERS, "n_rb %d not in [1,%d]", n_rb, SERL_MAX_BUFFERS);
  hipStream_t stream = (hipStream_t)stream_;
  serl_rb* r0 = rbs[0];
  SERL_REQUIRE(r0, "rbs[0] is NULL");
  const int T = r0->T, out_T = out->num_stack > 0 ? out->num_stack : 1;
  SERL_REQUIRE(T >= 1 && T <= kMaxStack, "fused gather+crop supports num_stack 1..%d (the store has %d)", kMaxStack, T);
  SERL_REQUIRE(out_T == T, "the store holds stacks of %d frames, serl_batch.num_stack is %d", T, out_T);
  int total = 0;
  for (int b = 0; b < n_rb; ++b) {
    SERL_REQUIRE(rbs[b] && host_idx[b], "NULL buffer/index");
    SERL_REQUIRE(counts[b] >= 0, "negative count");
    SERL_REQUIRE(rbs[b]->n_cam == r0->n_cam && rbs[b]->H == r0->H && rbs[b]->W == r0->W &&
                     rbs[b]->C == r0->C && rbs[b]->S == r0->S && rbs[b]->A == r0->A &&
                     rbs[b]->T == r0->T && rbs[b]->device == r0->device,
                 "buffers have different shapes");
    total += counts[b];
  }
  SERL_REQUIRE(total == out->batch && total > 0, "counts sum %d != batch %d", total, out->batch);
  SERL_REQUIRE(out->n_cam == r0->n_cam && (r0->n_cam == 0 || (out->H == r0->H && out->W == r0->W && out->C == r0->C)) &&
                   out->state_dim == T * r0->S && out->act_dim == r0->A, "serl_batch shape mismatch");
  SERL_REQUIRE((out->frames || r0->n_cam == 0) && out->state && out->action && out->reward && out->mask && out->done,
               "serl_batch has NULL outputs");
  RC(check_crops(host_crop_obs, total * T));
  RC(check_crops(host_crop_next, total * T));
  // lock all buffers (fixed order) while we read bookkeeping and enqueue
  Reader reader(rbs[0], n_rb == 2 && rbs[1] != rbs[0] ? rbs[1] : nullptr);
  std::unique_lock<std::mutex> l0(rbs[0]->mu, std::defer_lock), l1;
  if (n_rb == 2 && rbs[1] != rbs[0]) {
    l1 = std::unique_lock<std::mutex>(rbs[1]->mu, std::defer_lock);
    std::lock(l0, l1);
  } else {
    l0.lock();
  }
  SERL_HIP(hipSetDevice(r0->device));
  for (int b = 0; b < n_rb; ++b) {
    RC(check_and_revalidate(rbs[b], host_idx[b], counts[b]));
    RC(order_after_inserts(rbs[b], stream));
  }
  const size_t cbytes = sizeof(int32_t) * 2 * (size_t)total * T;
  const void* srcs[4] = {host_idx[0], n_rb > 1 ? host_idx[1] : nullptr, host_crop_obs, host_crop_next};
  size_t sizes[4] = {sizeof(int64_t) * (size_t)counts[0], n_rb > 1 ? sizeof(int64_t) * (size_t)counts[1] : 0,
                     host_crop_obs ? cbytes : 0, host_crop_next ? cbytes : 0}, offs[4];
  uint8_t* dparams;
  RC(stage_params(r0->stage, srcs, sizes, 4, stream, &dparams, offs));
  GatherArgs a{};
  for (int b = 0; b < n_rb; ++b) {
    for (int c = 0; c < r0->n_cam; ++c) a.frames[b][c] = rbs[b]->frames[c];
    a.rec[b] = rbs[b]->rec;
    a.cap[b] = rbs[b]->ix.cap;
    a.idx[b] = reinterpret_cast<const int64_t*>(dparams + offs[b]);
  }
  a.count0 = counts[0];
  a.batch = total; a.n_cam = r0->n_cam; a.H = r0->H; a.W = r0->W; a.C = r0->C; a.S = T * r0->S; a.A = r0->A; a.T = T;
  a.rec_len = r0->rec_len;
  a.crop_obs = host_crop_obs ? reinterpret_cast<const int32_t*>(dparams + offs[2]) : nullptr;
  a.crop_next = host_crop_next ? reinterpret_cast<const int32_t*>(dparams + offs[3]) : nullptr;
  a.out_frames = out->frames; a.out_state = out->state; a.out_action = out->action;
  a.out_reward = out->reward; a.out_mask = out->mask; a.out_done = out->done;
  a.from_packed = 0;
  RC(launch_gather_crop(a, stream));
  RC(r0->stage.mark(stream));
  for (int b = 0; b < n_rb; ++b) RC(note_gather(rbs[b], stream));
  return SERL_OK;
}

// Standalone crop needs its own parameter staging (no buffer handle): one static ring, made at the first call.
static struct { std::mutex mu; int device = -1; StageRing ring; } g_crop;

int serl_crop_packed(int device, const uint8_t* const* dev_packed, int n_cam, int batch, int H,
                     int W, int C, const int32_t* host_crop_obs, const int32_t* host_crop_next,
                     uint8_t* dev_frames_out, void* stream_) {
  return serl_crop_packed_stacked(device, dev_packed, n_cam, batch, 1, H, W, C, host_crop_obs, host_crop_next, dev_frames_out, stream_);
}

int serl_crop_packed_stacked(int device, const uint8_t* const* dev_packed, int n_cam, int batch, int num_stack, int H,
                             int W, int C, const int32_t* host_crop_obs, const int32_t* host_crop_next,
                             uint8_t* dev_frames_out, void* stream_) {
  SERL_REQUIRE(dev_packed && dev_frames_out, "NULL argument");
  SERL_REQUIRE(n_cam >= 1 && n_cam <= SERL_MAX_CAMS && batch > 0, "bad n_cam/batch");
  SERL_REQUIRE(num_stack >= 1 && num_stack <= kMaxStack, "num_stack %d not in [1,%d]", num_stack, kMaxStack);
  const int T = num_stack;
  SERL_REQUIRE(((size_t)W * C) % 16 == 0, "W*C (%d) must be a multiple of 16 bytes", W * C);
  hipStream_t stream = (hipStream_t)stream_;
  std::lock_guard<std::mutex> g(g_crop.mu);
  SERL_HIP(hipSetDevice(device));
  if (g_crop.device != device) {
    SERL_REQUIRE(g_crop.device == -1, "serl_crop_packed is bound to device %d", g_crop.device);
    RC(g_crop.ring.init(kRing, 1 << 16, true));
    g_crop.device = device;
  }
  RC(check_crops(host_crop_obs, batch * T));  // every check comes before a staging slot is taken
  RC(check_crops(host_crop_next, batch * T));
  const size_t cbytes = sizeof(int32_t) * 2 * (size_t)batch * T;
  const void* srcs[2] = {host_crop_obs, host_crop_next};
  size_t sizes[2] = {cbytes, cbytes}, offs[2];  // both tables keep their place in the slot, given or not
  uint8_t* d;
  RC(stage_params(g_crop.ring, srcs, sizes, 2, stream, &d, offs));
  GatherArgs a{};
  for (int c = 0; c < n_cam; ++c) a.packed[c] = dev_packed[c];
  a.from_packed = 1;
  a.count0 = batch;
  a.batch = batch; a.n_cam = n_cam; a.H = H; a.W = W; a.C = C; a.T = T;
  a.crop_obs = host_crop_obs ? reinterpret_cast<const int32_t*>(d + offs[0]) : nullptr;
  a.crop_next = host_crop_next ? reinterpret_cast<const int32_t*>(d + offs[1]) : nullptr;
  a.out_frames = dev_frames_out;
  RC(launch_gather_crop(a, stream));
  return g_crop.ring.mark(stream);
}

}  // extern "C"
