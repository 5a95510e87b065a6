// Launch planner of the batched replay insert, with no HIP in it: it consumes the slot operations of ReplayIndex::plan_insert
// (replay_index.h) for the transitions of a payload, in order, and groups them into launches.  It never re-derives the
// bookkeeping.  Standard library only, so tests/replay_batch_main.cpp proves the grouping on the CPU; replay.hip fills the
// staging entries and runs one insert_scatter_kernel per launch.
//
// A launch is an op table plus a count of staging entries.  A staging entry holds one slot write: the record padded to 256
// bytes, then one frame per camera.  The ops of one launch run in NO defined order, so the launch is cut before an op if
//   * its dst is already a dst of the launch (a payload longer than the ring overwrites its own slots),
//   * its dst is a store slot that a copy op of the launch reads,
//   * it is a copy whose source the launch writes (the wrap re-insert copies slots cap-T..cap-1, which the same payload may
//     just have written), or
//   * the staging budget (entries, or places in the op table) is full.
// Every launch therefore has distinct dsts, none of which a copy of the same launch reads: executed in any order against the
// store as it was before the launch, it leaves what sequential execution leaves.
#pragma once
#include <cstdint>
#include <vector>

#include "replay_index.h"

namespace serl {

// One op of a launch, as the kernel reads it (32 bytes).  kind is SlotOp::Kind.  Writes: src = staging entry of the launch,
// frame = which frame of the transition's observation (kObsFrame) or next observation (kNextFrame) the entry holds, tr = the
// transition of the payload it belongs to -- the last two tell the host what to put into the entry.  Copies: src = store slot.
struct BatchOp {
  int32_t kind, frame;
  int64_t dst, src, tr;
};

struct BatchPlan {
  std::vector<BatchOp> ops;  // of the launch being built
  int entries = 0;           // staging entries it uses
  int max_entries = 1, max_ops = 1, T = 1;

  // max_entries: staging entries per launch (>= 1).  A launch of distinct dsts covers less than one turn of the ring, so it
  // holds at most the T copies of one wrap: the op table has max_entries + T places.
  void init(int64_t cap, int num_stack, int budget_entries) {
    T = num_stack;
    max_entries = budget_entries;
    max_ops = budget_entries + num_stack;
    ops.reserve((size_t)max_ops);
    wrote_.assign((size_t)cap, 0);
    read_.assign((size_t)cap, 0);
    launch_ = 1;
    clear_ops();
  }

  // may `op` join the launch being built?
  bool fits(const SlotOp& op) const {
    if (wrote_[op.dst] == launch_ || read_[op.dst] == launch_) return false;
    if (op.kind == SlotOp::kCopy) {
      if (wrote_[op.arg] == launch_) return false;
    } else if (entries == max_entries) {
      return false;
    }
    return (int)ops.size() < max_ops;
  }

  // `op` of transition `tr` joins the launch; if it may not, flush() -- which runs the launch built so far -- is called
  // first and a new launch begins.  -> flush()'s status if that is not 0, else 0.
  template <class Flush>
  int push(const SlotOp& op, int64_t tr, Flush&& flush) {
    if (!fits(op)) {
      if (const int rc = flush()) return rc;
      clear();
    }
    wrote_[op.dst] = launch_;
    if (op.kind == SlotOp::kCopy) {
      read_[op.arg] = launch_;
      ops.push_back(BatchOp{(int32_t)op.kind, 0, op.dst, op.arg, tr});
    } else {
      ops.push_back(BatchOp{(int32_t)op.kind, (int32_t)op.arg, op.dst, entries++, tr});
    }
    return 0;
  }

  // the slot writes of one more transition (at most T first-frame slots and its own) fit the entries that are left
  bool room_for_transition() const { return entries + T + 1 <= max_entries; }

  // after a launch has run: the next one starts empty
  void clear() {
    if (++launch_ == 0) {  // the stamps have wrapped
      wrote_.assign(wrote_.size(), 0);
      read_.assign(read_.size(), 0);
      launch_ = 1;
    }
    clear_ops();
  }

 private:
  void clear_ops() { ops.clear(); entries = 0; }
  std::vector<uint32_t> wrote_, read_;  // per store slot: the launch that last wrote / copied from it
  uint32_t launch_ = 1;
};

}  // namespace serl
