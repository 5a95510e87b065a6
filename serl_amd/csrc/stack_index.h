// Index arithmetic of the fused gather + crop for frame stacks (num_stack = T frames per observation), with no HIP in it: which
// frame a workgroup of gather_crop_kernel / gather_crop_rgb_kernel serves, where that frame comes from and where it goes.
// The kernels in replay.hip call these functions; tests/stack_index_main.cpp drives the same code on the CPU under the host
// sanitizers.  Reference: utils/train_utils.py:53-64 (_unpack: observation = frames 0..T-1 of the packed T+1 window, next
// observation = frames 1..T), vision/data_augmentations.py:22-36 (batched_random_crop with num_batch_dims=2: frame (b, t) takes
// key b*T + t), data/memory_efficient_replay_buffer.py:149-153 (the window of a slot, and numpy's wrap of a negative one).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SERL_HD __host__ __device__ __forceinline__
#else
#define SERL_HD inline
#endif

namespace serl {

// frame workgroup -> (part of the frame, stack frame t, sample i, camera, which: 0 = observation, 1 = next), part fastest.
// With T == 1 this is the single-frame decode: t = 0 and the same (part, i, cam, which).
struct StackJob { int part, t, i, cam, which; };
SERL_HD StackJob stack_job(int bid, int parts, int T, int batch, int n_cam) {
  StackJob j;
  j.part = bid % parts; bid /= parts;
  j.t = bid % T; bid /= T;
  j.i = bid % batch; bid /= batch;
  j.cam = bid % n_cam;
  j.which = bid / n_cam;
  return j;
}
SERL_HD int64_t stack_frame_blocks(int parts, int T, int batch, int n_cam) { return 2LL * n_cam * batch * T * parts; }
// the frame's place in out_frames u8[2][n_cam][batch][T][frame]
SERL_HD int64_t stack_dst_frame(const StackJob& j, int T, int batch, int n_cam) {
  return (((int64_t)j.which * n_cam + j.cam) * batch + j.i) * T + j.t;
}
// its entry in the crop table int32[batch*T][2]
SERL_HD int stack_crop_entry(const StackJob& j, int T) { return j.i * T + j.t; }
// its frame inside the packed window u8[batch][T+1][frame] (already-gathered batches) ...
SERL_HD int64_t stack_packed_frame(const StackJob& j, int T) { return (int64_t)j.i * (T + 1) + j.which + j.t; }
// ... and the slot of frame f (0..T) of the window of slot idx in a ring of cap slots: slots idx-T .. idx; numpy wraps a
// negative window index to cap - T + (idx - T) (reference quirk for a valid slot below T, oracle/replay_oracle.py gather())
SERL_HD int64_t window_slot(int64_t idx, int T, int64_t cap, int f) {
  int64_t start = idx - T;
  if (start < 0) start += cap - T;
  return start + f;
}

}  // namespace serl
