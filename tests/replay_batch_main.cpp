// Proves the launch-cut rule of serl_amd/csrc/replay_batch.h on the CPU, under the host sanitizers (tests/test_replay_batch_cpu.py
// builds and runs it).  A host model of the slots is fed one transition stream twice:
//   sequential: ReplayIndex::plan_insert per transition, each plan executed in order;
//   batched:    a second ReplayIndex feeds BatchPlan payload by payload; every launch is executed twice over, on two copies of the
//               slots, once in reverse and once in a seeded-shuffle op order, copy sources read from a snapshot taken before the
//               launch -- the ops of a launch run in no defined order on the device.
// After every payload the slots, valid mask, size, insert_index, insert_count and first of the three must be equal, and every
// launch must satisfy the cut conditions.  Usage: replay_batch_main <T | 0 for the frameless store>; one line per case.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "replay_batch.h"

using serl::BatchOp;
using serl::BatchPlan;
using serl::ReplayIndex;
using serl::SlotOp;

struct Cell {
  int64_t rec = -1, frame = -1;  // which transition's record / which frame of it the slot holds
  bool operator==(const Cell& o) const { return rec == o.rec && frame == o.frame; }
};
static Cell written(const SlotOp::Kind kind, int64_t arg, int64_t tr) { return Cell{tr, (tr << 4) | ((int64_t)kind << 3) | arg}; }

#define CHECK(cond, ...)                                                     \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond);           \
      std::printf(__VA_ARGS__);                                              \
      std::printf("\n");                                                     \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

struct Batched {
  ReplayIndex ix;
  BatchPlan plan;
  std::vector<Cell> rev, shuf, staging;  // the two copies of the slots; the staging entries of the launch being built
  std::mt19937_64 rng{7};
  int64_t launches = 0, ops_run = 0, most_copies = 0;

  void check_cut_conditions() const {
    const std::vector<BatchOp>& ops = plan.ops;
    CHECK(!ops.empty() && (int)ops.size() <= plan.max_ops && plan.entries <= plan.max_entries, "%zu ops, %d entries", ops.size(),
          plan.entries);
    int entries = 0;
    for (size_t i = 0; i < ops.size(); ++i) {
      CHECK(ops[i].dst >= 0 && ops[i].dst < ix.cap, "dst %lld", (long long)ops[i].dst);
      if (ops[i].kind == SlotOp::kCopy) CHECK(ops[i].src >= 0 && ops[i].src < ix.cap, "copy source %lld", (long long)ops[i].src);
      else CHECK(ops[i].src == entries++, "write %zu reads entry %lld, not %d", i, (long long)ops[i].src, entries - 1);
      for (size_t j = 0; j < ops.size(); ++j) {
        CHECK(i == j || ops[i].dst != ops[j].dst, "ops %zu and %zu both write slot %lld", i, j, (long long)ops[i].dst);
        CHECK(ops[j].kind != SlotOp::kCopy || ops[j].src != ops[i].dst, "op %zu copies slot %lld, which op %zu writes", j,
              (long long)ops[j].src, i);
      }
    }
    CHECK(entries == plan.entries, "%d writes, %d entries", entries, plan.entries);
  }

  int run_launch() {
    check_cut_conditions();
    std::vector<size_t> order(plan.ops.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = order.size() - 1 - i;
    for (std::vector<Cell>* slots : {&rev, &shuf}) {
      const std::vector<Cell> before = *slots;
      for (size_t i : order) {
        const BatchOp& op = plan.ops[i];
        (*slots)[op.dst] = op.kind == SlotOp::kCopy ? before[op.src] : staging[op.src];
      }
      std::shuffle(order.begin(), order.end(), rng);
    }
    int64_t copies = 0;
    for (const BatchOp& op : plan.ops) copies += op.kind == SlotOp::kCopy;
    most_copies = std::max(most_copies, copies);
    launches += 1;
    ops_run += (int64_t)plan.ops.size();
    return 0;
  }

  // as serl_rb_insert_batch: the transitions of a payload in order; a launch also ends where the next transition might not fit
  // (`release`: the store's mutex is released there) and at the end of the payload
  void insert(const std::vector<uint8_t>& done, int64_t first_tr, bool release) {
    for (size_t i = 0; i < done.size(); ++i) {
      for (const SlotOp& op : ix.plan_insert(done[i] != 0)) {
        const bool cut = !plan.fits(op);
        const size_t before = plan.ops.size();
        plan.push(op, (int64_t)i, [this] { return run_launch(); });
        CHECK(cut ? plan.ops.size() == 1 : plan.ops.size() == before + 1, "push after %zu ops left %zu", before, plan.ops.size());
        const BatchOp& b = plan.ops.back();
        CHECK(b.tr == (int64_t)i && b.dst == op.dst && b.kind == op.kind, "op does not carry the plan's");
        if (op.kind != SlotOp::kCopy) staging[b.src] = written(op.kind, b.frame, first_tr + b.tr);
      }
      if (release && !plan.room_for_transition() && i + 1 < done.size()) {
        run_launch();
        plan.clear();
      }
    }
    if (!plan.ops.empty()) {
      run_launch();
      plan.clear();
    }
  }
};

static void run_case(int64_t cap, bool frames, int T, int budget, bool release) {
  ReplayIndex seq;
  seq.init(cap, frames, T);
  std::vector<Cell> slots((size_t)cap);
  Batched b;
  b.ix.init(cap, frames, T);
  b.plan.init(cap, T, budget);
  b.rev.assign((size_t)cap, Cell());
  b.shuf.assign((size_t)cap, Cell());
  b.staging.assign((size_t)budget, Cell());
  std::mt19937_64 rng((uint64_t)(cap * 131 + T * 17 + budget));
  const int64_t sizes[6] = {1, 2, 7, cap - 1, cap, 2 * cap + 3};
  int64_t total = 0, payloads = 0;
  while (total < 2000 || payloads % 6 != 0) {
    const int64_t n = sizes[payloads++ % 6];
    std::vector<uint8_t> done((size_t)n);
    for (uint8_t& d : done) d = (rng() % 5) == 0;  // done probability 0.2
    for (int64_t i = 0; i < n; ++i)
      for (const SlotOp& op : seq.plan_insert(done[(size_t)i] != 0))
        slots[op.dst] = op.kind == SlotOp::kCopy ? slots[op.arg] : written(op.kind, op.arg, total + i);
    b.insert(done, total, release);
    total += n;
    CHECK(b.ix.size == seq.size && b.ix.insert_index == seq.insert_index && b.ix.insert_count == seq.insert_count &&
              b.ix.first == seq.first && b.ix.valid == seq.valid, "bookkeeping differs after payload %lld", (long long)payloads);
    for (int64_t s = 0; s < cap; ++s)
      CHECK(b.rev[s] == slots[s] && b.shuf[s] == slots[s], "slot %lld differs after payload %lld of %lld (reverse: frame %lld, shuffled: "
            "frame %lld, sequential: frame %lld)", (long long)s, (long long)payloads, (long long)n, (long long)b.rev[s].frame,
            (long long)b.shuf[s].frame, (long long)slots[s].frame);
  }
  CHECK(b.ops_run == seq.insert_count, "%lld ops run, %lld slot writes", (long long)b.ops_run, (long long)seq.insert_count);
  CHECK(b.most_copies <= T, "%lld copies in one launch", (long long)b.most_copies);
  std::printf("case cap=%lld frames=%d T=%d budget=%d release=%d transitions=%lld launches=%lld\n", (long long)cap, (int)frames, T, budget,
              (int)release, (long long)total, (long long)b.launches);
}

int main(int argc, char** argv) {
  const int T = argc > 1 ? std::atoi(argv[1]) : -1;
  if (T < 0 || T > 4) {
    std::printf("usage: replay_batch_main <T 1..4 | 0 for the frameless store>\n");
    return 2;
  }
  const int64_t frame_caps[3] = {3 * T + 2, 11 + T, 37}, plain_caps[3] = {2, 5, 16};
  const int64_t* caps = T ? frame_caps : plain_caps;
  for (int c = 0; c < 3; ++c)
    for (int budget : {1, 3, 64})
      for (bool release : {false, true}) run_case(caps[c], T != 0, T ? T : 1, budget, release);
  std::printf("ok\n");
  return 0;
}
