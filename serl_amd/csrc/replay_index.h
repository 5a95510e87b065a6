// Host bookkeeping of the replay store, with no HIP in it: the reference's slot bookkeeping
// (serl_launcher/data/memory_efficient_replay_buffer.py:53-89, replay_buffer.py:71-75) and a bit-exact PCG64/Lemire
// index sampler (numpy Generator.integers; memory_efficient_replay_buffer.py:111-122).  Standard library only, so
// tests/replay_index_main.cpp drives it on the CPU; replay.hip does the staging, the stream ordering and the kernels.
#pragma once
#include <cstdint>
#include <vector>

namespace serl {

// ---------------------------------------------------------------------------------------------
// PCG64 XSL-RR 128/64 with numpy's buffered next_uint32 and Lemire bounded draws.
// ---------------------------------------------------------------------------------------------
struct Pcg64 {
  unsigned __int128 state = 0, inc = 0;
  int has_uint32 = 0;
  uint32_t uinteger = 0;
  bool seeded = false;

  uint64_t next64() {
    const unsigned __int128 mult =
        ((unsigned __int128)0x2360ED051FC65DA4ULL << 64) | 0x4385DF649FCCF645ULL;
    state = state * mult + inc;
    uint64_t hi = (uint64_t)(state >> 64), lo = (uint64_t)state;
    uint64_t x = hi ^ lo;
    unsigned r = (unsigned)(state >> 122);
    return (x >> r) | (x << ((64 - r) & 63));
  }
  uint32_t next32() {
    if (has_uint32) {
      has_uint32 = 0;
      return uinteger;
    }
    uint64_t v = next64();
    has_uint32 = 1;
    uinteger = (uint32_t)(v >> 32);
    return (uint32_t)v;
  }
  // Generator.integers(n), 0 < n < 2^32 - 1 (numpy buffered_bounded_lemire_uint32)
  uint32_t bounded(uint32_t n) {
    if (n == 1) return 0;
    uint64_t m = (uint64_t)next32() * n;
    uint32_t l = (uint32_t)m;
    if (l < n) {
      uint32_t t = (0xFFFFFFFFu - (n - 1)) % n;
      while (l < t) {
        m = (uint64_t)next32() * n;
        l = (uint32_t)m;
      }
    }
    return (uint32_t)(m >> 32);
  }
  // the 128-bit state and increment as {state hi, state lo, inc hi, inc lo}
  void get(uint64_t out[4]) const {
    out[0] = (uint64_t)(state >> 64); out[1] = (uint64_t)state;
    out[2] = (uint64_t)(inc >> 64); out[3] = (uint64_t)inc;
  }
  void set(const uint64_t in[4], int has, uint32_t uint) {
    state = ((unsigned __int128)in[0] << 64) | in[1];
    inc = ((unsigned __int128)in[2] << 64) | in[3];
    has_uint32 = has;
    uinteger = uint;
    seeded = true;
  }
};

// The ring range [slot_begin, slot_begin + n_slots) mod cap as at most two runs of consecutive slots: (first slot, slots, position
// of the run in the caller's arrays).
struct SlotRun { int64_t slot, n, at; };

// One slot operation of an insert.  kCopy: copy slot `arg` to slot `dst` (wrap re-insert); kObsFrame: write frame `arg` of the
// observation and the record to `dst` (first-frame slot); kNextFrame: write frame `arg` (= T-1) of the next observation and the
// record to `dst`.
struct SlotOp {
  enum Kind { kCopy, kObsFrame, kNextFrame } kind;
  int64_t dst, arg;
};

enum class IndexStatus { kOk, kNotSeeded, kEmpty, kNoneValid, kOutOfRange, kRedrawExhausted, kInconsistent };

// Not thread-safe: the caller holds the store's mutex.
struct ReplayIndex {
  int64_t cap = 0;
  bool has_frames = true;  // false: plain ReplayBuffer of flat observations, every inserted slot is valid
  int T = 1;
  std::vector<uint8_t> valid;
  int64_t size = 0, insert_index = 0;
  int64_t insert_count = 0;  // slot writes ever made (insert_index == insert_count % cap)
  bool first = true;
  Pcg64 rng;
  std::vector<SlotOp> plan;  // of the last plan_insert

  void init(int64_t capacity, bool frames, int num_stack) {
    cap = capacity; has_frames = frames; T = num_stack;
    valid.assign((size_t)capacity, 0);
    plan.reserve(2 * (size_t)num_stack + 1);
  }

  // The slot operations of inserting one transition, at most 2T + 1, in order.  The bookkeeping is complete when this returns
  // (each operation's validity bit applied, the head advanced): whoever moves the data executes the plan and never re-derives it.
  const std::vector<SlotOp>& plan_insert(bool done) {
    plan.clear();
    if (!has_frames) {  // ReplayBuffer.insert (replay_buffer.py:71-75): write at the head, advance, no bookkeeping
      valid[insert_index] = 1;
      plan.push_back({SlotOp::kNextFrame, advance(), T - 1});
      return plan;
    }
    // wrap: re-insert the last T slots at the head as invalid (py:54-59)
    if (insert_index == 0 && cap == size && !first) {
      for (int64_t src = size - T; src < size; ++src) {
        valid[insert_index] = 0;
        plan.push_back({SlotOp::kCopy, advance(), src});
      }
    }
    if (first) {  // episode start: T invalid "first-frame" slots holding the obs frames (py:71-77)
      for (int t = 0; t < T; ++t) {
        valid[insert_index] = 0;
        plan.push_back({SlotOp::kObsFrame, advance(), t});
      }
    }
    first = done;
    valid[insert_index] = 1;
    plan.push_back({SlotOp::kNextFrame, advance(), T - 1});
    for (int t = 0; t < T; ++t) valid[(insert_index + t) % size] = 0;  // py:87-89
    return plan;
  }

  // integers(len, size=batch), then the rejection loop over invalid slots
  IndexStatus sample(int batch, int64_t* out) {
    if (!rng.seeded) return IndexStatus::kNotSeeded;
    if (batch <= 0) return IndexStatus::kOk;
    if (size <= 0) return IndexStatus::kEmpty;
    bool any = false;
    for (int64_t i = 0; i < size && !any; ++i) any = valid[i];
    if (!any) return IndexStatus::kNoneValid;
    const uint32_t n = (uint32_t)size;
    for (int i = 0; i < batch; ++i) out[i] = rng.bounded(n);
    for (int i = 0; i < batch; ++i)
      while (!valid[out[i]]) out[i] = rng.bounded(n);
    return IndexStatus::kOk;
  }

  // The reference holds one lock across index draw and gather (data_store.py:108-111); here they are two calls (the
  // lazy / prefetched path), so an insert in between may have invalidated a drawn slot (the look-ahead invalidation of
  // memory_efficient_replay_buffer.py:87-89, a new episode's first-frame slot, the wrap re-insert).  A slot that is still
  // valid pairs with slot-1 consistently (writes are sequential), so validity is the whole check: stale indices are
  // re-drawn from the buffer's generator, exactly as the rejection loop would have, IN PLACE: the caller's array then
  // describes the batch that is actually gathered (index-keyed bookkeeping and determinism checks stay valid).
  IndexStatus revalidate(int64_t* idx, int n) {
    if (!has_frames) return IndexStatus::kOk;  // plain ReplayBuffer: every slot below `size` is valid
    for (int i = 0; i < n; ++i) {
      if (valid[idx[i]]) continue;
      if (!rng.seeded) return IndexStatus::kNotSeeded;
      const uint32_t sz = (uint32_t)size;
      int guard = 0;
      do {
        idx[i] = rng.bounded(sz);
        if (++guard >= (1 << 24)) return IndexStatus::kRedrawExhausted;
      } while (!valid[idx[i]]);
    }
    return IndexStatus::kOk;
  }

  // every index in [0, size); *bad is the position of the first that is not
  IndexStatus check_indices(const int64_t* idx, int n, int* bad) const {
    for (int i = 0; i < n; ++i)
      if (idx[i] < 0 || idx[i] >= size) { *bad = i; return IndexStatus::kOutOfRange; }
    return IndexStatus::kOk;
  }

  int slot_runs(int64_t slot_begin, int64_t n_slots, SlotRun runs[2]) const {
    const int64_t head = n_slots < cap - slot_begin ? n_slots : cap - slot_begin;
    int k = 0;
    if (head > 0) runs[k++] = SlotRun{slot_begin, head, 0};
    if (n_slots - head > 0) runs[k++] = SlotRun{0, n_slots - head, head};
    return k;
  }

  // takes over a snapshot's bookkeeping if it is consistent at this capacity
  IndexStatus restore(int64_t size_, int64_t insert_index_, int64_t insert_count_, bool first_) {
    if (!(insert_count_ >= 0 && insert_index_ == insert_count_ % cap && size_ == (insert_count_ < cap ? insert_count_ : cap)))
      return IndexStatus::kInconsistent;
    size = size_; insert_index = insert_index_; insert_count = insert_count_; first = first_;
    return IndexStatus::kOk;
  }

 private:
  int64_t advance() {  // -> the slot at the head, which moves on
    const int64_t i = insert_index;
    insert_index = (i + 1) % cap;
    insert_count += 1;
    size = size + 1 < cap ? size + 1 : cap;
    return i;
  }
};

}  // namespace serl
