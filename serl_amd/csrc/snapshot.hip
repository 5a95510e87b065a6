// Parameter snapshots: a consistent copy of a serl_agent's train state, taken on the update stream in ONE launch and moved to
// pinned host memory behind the learner's back (include/serl_mi355.h "Parameter snapshots").  The reference's learner loop sends
// its parameters to the actor every 30 iterations and writes a checkpoint every few thousand
// (examples/async_drq_sim/async_drq_sim.py:229,295-307); serl_agent_get serves that with one blocking copy per leaf.
//
// take:   [update stream]  memset of the slot's counters -> snapshot_pack_kernel (arena -> device staging slot) -> event
//         [copy stream]    wait on that event -> one D2H of the whole slot into its pinned twin -> event
// The updates enqueued behind the take start as soon as the pack kernel is done: the D2H reads the staging copy, never the arena.
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "internal.h"
#include "snapshot_plan.h"

using namespace serl;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kPackVec = 4;   // 16-byte loads in flight per thread before its first store
static_assert(kSnapPartFloats == 256L * kPackVec * 4, "a part is what one 256-thread workgroup moves with kPackVec vectors per thread");

__device__ __forceinline__ int nonfinite(float x) {   // exponent bits all ones: Inf or NaN
  return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u;
}

// One workgroup per part (snapshot_plan.h).  No LDS and a handful of registers: the kernel runs beside two resident trunk
// workgroups.  The non-finite count is reduced over the wave by shuffles; the waves of a workgroup share
// no LDS to combine in, so each wave that FOUND something adds its count with one ordinary global atomic -- a finite state, the
// only one that is published, issues no atomic at all.
__global__ __launch_bounds__(256) void snapshot_pack_kernel(const SnapPartDev* __restrict__ parts, uint8_t* __restrict__ slot) {
  const SnapPartDev p = parts[blockIdx.x];
  const int tid = threadIdx.x;
  // (a pointer read from memory is a generic one to the compiler: say that it is global, for global_load instead of flat_load)
  typedef const float __attribute__((address_space(1))) * GlobalF;
  typedef const f32x4 __attribute__((address_space(1))) * GlobalV;
  const GlobalF srcf = (GlobalF)(uintptr_t)p.src;
  const GlobalV src = (GlobalV)srcf;
  f32x4* dst = reinterpret_cast<f32x4*>(slot + p.dst);
  const int nvec = p.len >> 2;
  f32x4 v[kPackVec];
#pragma unroll
  for (int j = 0; j < kPackVec; ++j) {
    const int i = j * 256 + tid;
    v[j] = i < nvec ? src[i] : (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  int bad = 0;
#pragma unroll
  for (int j = 0; j < kPackVec; ++j) {
    const int i = j * 256 + tid;
    bad += nonfinite(v[j][0]) + nonfinite(v[j][1]) + nonfinite(v[j][2]) + nonfinite(v[j][3]);
    if (i < nvec) __builtin_nontemporal_store(v[j], dst + i);   // nothing on the device reads the staging copy but the D2H
  }
  const int tail = p.len & 3;
  if (tid < tail) {   // fewer than four floats behind the last whole vector of a run
    const float x = srcf[(nvec << 2) + tid];
    bad += nonfinite(x);
    reinterpret_cast<float*>(dst)[(nvec << 2) + tid] = x;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) bad += __shfl_xor(bad, m, 64);
  if ((tid & 63) == 0 && bad) atomicAdd(reinterpret_cast<unsigned int*>(slot) + p.section, (unsigned int)bad);
}

enum SlotState { kFree = 0, kHeld = 1 };

struct Slot {
  uint8_t* dev = nullptr;    // device staging copy
  uint8_t* host = nullptr;   // its pinned twin
  hipEvent_t packed = nullptr, copied = nullptr;
  int state = kFree;
  bool in_flight = false;    // a D2H was enqueued and `copied` not yet seen complete
  int64_t step = 0, trunk_gen = 0;
};

struct LeafAt {
  long off;     // byte offset in the slot, -1: outside the optimizer's support (reads as zeros)
  long count;
};

}  // namespace

struct serl_snapshot {
  serl_agent* agent = nullptr;
  int device = 0, sections = 0;
  SnapPlan plan;
  SnapPartDev* parts_dev = nullptr;
  std::map<std::string, LeafAt> leaves;   // "section\nleaf"
  std::vector<float> zeros;               // what a moment outside its optimizer's support reads as
  std::vector<Slot> slots;
  hipStream_t copy_stream = nullptr;
  std::mutex mu;                          // slot states: take on the learner's thread, wait / leaf / release on the consumer's
};

namespace {

const char* const kSectionNames[] = {"params", "target_params"};
const char* const kOptSections[] = {"opt/actor/mu", "opt/actor/nu", "opt/critic/mu", "opt/critic/nu", "opt/temperature/mu", "opt/temperature/nu"};

void free_all(serl_snapshot* s) {
  for (Slot& t : s->slots) {
    if (t.copied) (void)hipEventDestroy(t.copied);
    if (t.packed) (void)hipEventDestroy(t.packed);
    if (t.host) (void)hipHostFree(t.host);
    if (t.dev) (void)hipFree(t.dev);
  }
  if (s->copy_stream) (void)hipStreamDestroy(s->copy_stream);
  if (s->parts_dev) (void)hipFree(s->parts_dev);
  delete s;
}

// has the slot's last D2H finished?  (clears in_flight once it has)
int copy_done(Slot& t, bool* done) {
  *done = true;
  if (!t.in_flight) return SERL_OK;
  const hipError_t e = hipEventQuery(t.copied);
  if (e == hipErrorNotReady) { *done = false; return SERL_OK; }
  SERL_HIP(e);
  t.in_flight = false;
  return SERL_OK;
}

int check_slot(serl_snapshot* s, int slot, const char* what) {
  SERL_REQUIRE(s, "NULL snapshot handle");
  SERL_REQUIRE(slot >= 0 && slot < (int)s->slots.size(), "%s: slot %d not in [0, %d)", what, slot, (int)s->slots.size());
  return SERL_OK;
}

int not_held(const char* what, int slot) {
  set_error("%s: slot %d holds no snapshot (never taken, or released)", what, slot);
  return SERL_ERR_STATE;
}

}  // namespace

int serl_snapshot_create(serl_agent* a, int sections, int slots, serl_snapshot** out) {
  SERL_REQUIRE(a && out, "NULL argument");
  SERL_REQUIRE(sections > 0 && (sections & ~(SERL_SNAP_PARAMS | SERL_SNAP_TARGET | SERL_SNAP_OPT)) == 0,
               "sections %d: a non-empty combination of SERL_SNAP_PARAMS (1), SERL_SNAP_TARGET (2) and SERL_SNAP_OPT (4)", sections);
  SERL_REQUIRE(slots >= 1 && slots <= 4, "slots %d not in [1, 4]", slots);
  SERL_HIP(hipSetDevice(agent_device(a)));
  // every (section, leaf) of the leaf table, resolved once
  struct Want { std::string section, leaf; int sec; float* p; long n; };
  std::vector<Want> want;
  char name[160];
  int64_t cnt = 0;
  for (int i = 0, n = serl_agent_num_leaves(a); i < n; ++i) {
    RC(serl_agent_leaf_info(a, i, name, sizeof(name), &cnt));
    for (int sec = 0; sec < kSnapSections; ++sec) {
      if (!(sections & (1 << sec))) continue;
      const char* const* names = sec < 2 ? &kSectionNames[sec] : kOptSections;
      for (int k = 0, nk = sec < 2 ? 1 : 6; k < nk; ++k) {
        Want w{names[k], name, sec, nullptr, 0};
        RC(agent_resolve(a, names[k], name, &w.p, &w.n));
        want.push_back(w);
      }
    }
  }
  // their maximal contiguous runs, section by section, laid out back to back
  std::vector<SnapRun> runs;
  std::vector<uintptr_t> run_addr;
  for (int sec = 0; sec < kSnapSections; ++sec) {
    std::vector<SnapRange> r;
    for (const Want& w : want)
      if (w.sec == sec && w.p) r.push_back({reinterpret_cast<uintptr_t>(w.p), w.n});
    for (const SnapRange& m : snap_merge(r)) {
      if (m.addr & 15) {
        set_error("a run of section %d starts at device address %p, not a multiple of 16 bytes", sec, (void*)m.addr);
        return SERL_ERR_UNSUPPORTED;
      }
      runs.push_back({m.len, sec});
      run_addr.push_back(m.addr);
    }
  }
  serl_snapshot* s = new serl_snapshot();
  s->agent = a;
  s->device = agent_device(a);
  s->sections = sections;
  s->plan = snapshot_plan(runs);
  long zeros = 0;
  for (const Want& w : want) {
    LeafAt at{-1, w.n};
    if (w.p) {
      const uintptr_t p = reinterpret_cast<uintptr_t>(w.p);
      for (size_t r = 0; r < runs.size(); ++r)
        if (runs[r].section == w.sec && p >= run_addr[r] && p < run_addr[r] + (uintptr_t)runs[r].len * sizeof(float))
          at.off = (long)(s->plan.run_dst[r] + (p - run_addr[r]));
    } else if (w.n > zeros) {
      zeros = w.n;
    }
    s->leaves[w.section + "\n" + w.leaf] = at;
  }
  s->zeros.assign((size_t)zeros, 0.f);
  std::vector<SnapPartDev> parts;
  for (const SnapPart& q : s->plan.parts)
    parts.push_back({reinterpret_cast<const float*>(run_addr[q.run]) + q.off, (uint64_t)q.dst, q.len, q.section});
#define SNAP_HIP(call)                                                                                      \
  do {                                                                                                      \
    hipError_t _e = (call);                                                                                 \
    if (_e != hipSuccess) {                                                                                 \
      set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__);                 \
      free_all(s);                                                                                          \
      return SERL_ERR_HIP;                                                                                  \
    }                                                                                                       \
  } while (0)
  if (!parts.empty()) {
    SNAP_HIP(hipMalloc(&s->parts_dev, parts.size() * sizeof(SnapPartDev)));
    SNAP_HIP(hipMemcpy(s->parts_dev, parts.data(), parts.size() * sizeof(SnapPartDev), hipMemcpyHostToDevice));
  }
  SNAP_HIP(hipStreamCreateWithFlags(&s->copy_stream, hipStreamNonBlocking));
  s->slots.resize(slots);
  for (Slot& t : s->slots) {
    SNAP_HIP(hipMalloc(&t.dev, s->plan.bytes));
    SNAP_HIP(hipMemset(t.dev, 0, s->plan.bytes));   // (the padding behind a run is never written by the kernel)
    SNAP_HIP(hipHostMalloc(&t.host, s->plan.bytes, hipHostMallocDefault));
    std::memset(t.host, 0, s->plan.bytes);
    SNAP_HIP(hipEventCreateWithFlags(&t.packed, hipEventDisableTiming));
    SNAP_HIP(hipEventCreateWithFlags(&t.copied, hipEventDisableTiming));
  }
#undef SNAP_HIP
  agent_snapshot_count(a, +1);
  *out = s;
  return SERL_OK;
}

int serl_snapshot_take(serl_snapshot* s, void* stream, int* slot_out) {
  SERL_REQUIRE(s && slot_out, "NULL argument");
  std::lock_guard<std::mutex> lock(s->mu);
  SERL_HIP(hipSetDevice(s->device));
  hipStream_t st = (hipStream_t)stream;
  if (st) {
    hipDevice_t dev = 0;
    SERL_HIP(hipStreamGetDevice(st, &dev));
    if ((int)dev != s->device) {
      set_error("serl_snapshot_take: the stream belongs to device %d, the agent lives on device %d", (int)dev, s->device);
      return SERL_ERR_STATE;
    }
  }
  int slot = -1, busy = 0;
  for (int i = 0; i < (int)s->slots.size() && slot < 0; ++i) {
    if (s->slots[i].state != kFree) continue;
    bool done;
    RC(copy_done(s->slots[i], &done));   // released early: its D2H may still be writing the pinned buffer
    if (done) slot = i; else ++busy;
  }
  if (slot < 0) {
    set_error("serl_snapshot_take: no free slot among %d (%d held until serl_snapshot_release, %d released with their copy still running)",
              (int)s->slots.size(), (int)s->slots.size() - busy, busy);
    return SERL_ERR_STATE;
  }
  Slot& t = s->slots[slot];
  if (s->sections & SERL_SNAP_TARGET) RC(agent_flush_target_trunk(s->agent, st));
  SERL_HIP(hipMemsetAsync(t.dev, 0, kSnapHeaderBytes, st));
  if (!s->plan.parts.empty()) {
    hipLaunchKernelGGL(snapshot_pack_kernel, dim3((unsigned)s->plan.parts.size()), dim3(256), 0, st, s->parts_dev, t.dev);
    SERL_HIP(hipGetLastError());
  }
  SERL_HIP(hipEventRecord(t.packed, st));
  SERL_HIP(hipStreamWaitEvent(s->copy_stream, t.packed, 0));
  SERL_HIP(hipMemcpyAsync(t.host, t.dev, s->plan.bytes, hipMemcpyDeviceToHost, s->copy_stream));
  SERL_HIP(hipEventRecord(t.copied, s->copy_stream));
  t.state = kHeld;
  t.in_flight = true;
  t.step = serl_agent_get_step(s->agent);
  t.trunk_gen = agent_trunk_gen(s->agent);
  *slot_out = slot;
  return SERL_OK;
}

int serl_snapshot_ready(serl_snapshot* s, int slot) {
  RC(check_slot(s, slot, "serl_snapshot_ready"));
  std::lock_guard<std::mutex> lock(s->mu);
  if (s->slots[slot].state != kHeld) return not_held("serl_snapshot_ready", slot);
  SERL_HIP(hipSetDevice(s->device));
  bool done;
  RC(copy_done(s->slots[slot], &done));
  return done ? 1 : 0;
}

int serl_snapshot_wait(serl_snapshot* s, int slot) {
  RC(check_slot(s, slot, "serl_snapshot_wait"));
  hipEvent_t ev;
  {
    std::lock_guard<std::mutex> lock(s->mu);
    if (s->slots[slot].state != kHeld) return not_held("serl_snapshot_wait", slot);
    if (!s->slots[slot].in_flight) return SERL_OK;
    ev = s->slots[slot].copied;
  }
  SERL_HIP(hipSetDevice(s->device));
  SERL_HIP(hipEventSynchronize(ev));   // outside the mutex: a take on the learner's thread never waits for a reader
  std::lock_guard<std::mutex> lock(s->mu);
  bool done;
  return copy_done(s->slots[slot], &done);
}

// the slot's pinned buffer once its copy is complete (else SERL_ERR_STATE)
static int ready_host(serl_snapshot* s, int slot, const char* what, const uint8_t** host, Slot** t_out) {
  Slot& t = s->slots[slot];
  if (t.state != kHeld) return not_held(what, slot);
  SERL_HIP(hipSetDevice(s->device));
  bool done;
  RC(copy_done(t, &done));
  if (!done) {
    set_error("%s: the copy of slot %d is still running (serl_snapshot_wait, or poll serl_snapshot_ready)", what, slot);
    return SERL_ERR_STATE;
  }
  *host = t.host;
  *t_out = &t;
  return SERL_OK;
}

int serl_snapshot_info(serl_snapshot* s, int slot, serl_snapshot_meta* out) {
  RC(check_slot(s, slot, "serl_snapshot_info"));
  SERL_REQUIRE(out, "NULL argument");
  std::lock_guard<std::mutex> lock(s->mu);
  const uint8_t* host;
  Slot* t;
  RC(ready_host(s, slot, "serl_snapshot_info", &host, &t));
  out->step = t->step;
  out->trunk_gen = t->trunk_gen;
  out->bytes = (int64_t)s->plan.bytes;
  uint32_t c[kSnapSections];
  std::memcpy(c, host, sizeof(c));
  for (int i = 0; i < kSnapSections; ++i) out->nonfinite[i] = c[i];
  out->sections = s->sections;
  out->slots = (int)s->slots.size();
  return SERL_OK;
}

int serl_snapshot_leaf(serl_snapshot* s, int slot, const char* section, const char* leaf, const float** host_out, int64_t* count) {
  RC(check_slot(s, slot, "serl_snapshot_leaf"));
  SERL_REQUIRE(section && leaf && host_out && count, "NULL argument");
  std::lock_guard<std::mutex> lock(s->mu);
  const auto it = s->leaves.find(std::string(section) + "\n" + leaf);
  SERL_REQUIRE(it != s->leaves.end(), "the snapshot holds no leaf '%s' of section '%s' (sections mask %d)", leaf, section, s->sections);
  const uint8_t* host;
  Slot* t;
  RC(ready_host(s, slot, "serl_snapshot_leaf", &host, &t));
  *host_out = it->second.off < 0 ? s->zeros.data() : reinterpret_cast<const float*>(host + it->second.off);
  *count = it->second.count;
  return SERL_OK;
}

int serl_snapshot_release(serl_snapshot* s, int slot) {
  RC(check_slot(s, slot, "serl_snapshot_release"));
  std::lock_guard<std::mutex> lock(s->mu);
  if (s->slots[slot].state != kHeld) return not_held("serl_snapshot_release", slot);
  s->slots[slot].state = kFree;   // (in_flight stays: take passes over the slot until its copy has ended)
  return SERL_OK;
}

int serl_snapshot_destroy(serl_snapshot* s) {
  if (!s) return SERL_OK;
  (void)hipSetDevice(s->device);
  if (s->copy_stream) (void)hipStreamSynchronize(s->copy_stream);
  for (Slot& t : s->slots)
    if (t.packed) (void)hipEventSynchronize(t.packed);   // a pack kernel still queued on the caller's stream writes t.dev
  agent_snapshot_count(s->agent, -1);
  free_all(s);
  return SERL_OK;
}
