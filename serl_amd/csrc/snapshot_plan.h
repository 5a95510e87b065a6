// Staging layout and workgroup parts of a parameter snapshot (snapshot.hip): host arithmetic only, no device API, so that
// tests/snapshot_plan_main.cpp can prove it on the CPU under the host sanitizers (tests/test_snapshot_plan_cpu.py).
//
// A snapshot copies RUNS -- maximal contiguous float ranges of the agent's arena, each tagged with the section it belongs
// to -- into one staging slot:
//   [ header: one non-finite counter per section, kSnapHeaderBytes ][ run 0 ][ run 1 ] ...
// every run starting at a multiple of 16 bytes.  One workgroup of snapshot_pack_kernel moves one PART: at most kSnapPartFloats
// (16 KB: 256 threads x four 16-byte vectors) of one run, as a vector body of whole 16-byte vectors followed by a scalar tail of
// fewer than four floats (only the last part of a run has one).  A run's source must start at a multiple of 16 bytes too
// (snapshot.hip checks it); part offsets are multiples of 16 KB, so every body is aligned on both sides.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace serl {

constexpr int kSnapSections = 3;           // params, target_params, opt: bit i of the SERL_SNAP_* mask is section i
constexpr long kSnapPartFloats = 4096;     // floats of a full part
constexpr size_t kSnapHeaderBytes = 64;    // uint32 nonfinite[kSnapSections], padded so that the first run is 16-byte aligned

struct SnapRun {
  long len;      // floats, > 0
  int section;   // 0 .. kSnapSections - 1
};

struct SnapPart {
  int run;       // index into the run table
  int section;   // the run's section: which counter the part's non-finite count goes to
  long off;      // first float of the part inside its run (a multiple of kSnapPartFloats)
  int len;       // floats of the part, 1 .. kSnapPartFloats
  int body;      // floats moved as 16-byte vectors: len rounded down to a multiple of 4
  int tail;      // floats moved one by one behind the body: len - body, 0 .. 3
  size_t dst;    // byte offset of the part in the staging slot
};

struct SnapPlan {
  std::vector<size_t> run_dst;   // byte offset of every run in the staging slot
  std::vector<SnapPart> parts;   // run by run, in offset order
  size_t bytes = 0;              // the staging slot: header + every run rounded up to 16 bytes
};

inline size_t snap_round16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

inline SnapPlan snapshot_plan(const std::vector<SnapRun>& runs) {
  SnapPlan p;
  size_t at = kSnapHeaderBytes;
  for (size_t r = 0; r < runs.size(); ++r) {
    p.run_dst.push_back(at);
    for (long off = 0; off < runs[r].len; off += kSnapPartFloats) {
      const long left = runs[r].len - off;
      SnapPart q;
      q.run = (int)r;
      q.section = runs[r].section;
      q.off = off;
      q.len = (int)(left < kSnapPartFloats ? left : kSnapPartFloats);
      q.body = q.len & ~3;
      q.tail = q.len - q.body;
      q.dst = at + (size_t)off * sizeof(float);
      p.parts.push_back(q);
    }
    at += snap_round16((size_t)runs[r].len * sizeof(float));
  }
  p.bytes = at;
  return p;
}

// One part as the kernel reads it (the device copy of the part table): source address, byte offset in the slot, floats, section.
struct SnapPartDev {
  const float* src;
  uint64_t dst;
  int32_t len;
  int32_t section;
};

// [first, first + count) float ranges -> their maximal contiguous runs, in address order.  `r` holds (address in bytes, floats);
// ranges of one section never overlap (they are distinct leaves of one arena).
struct SnapRange {
  uintptr_t addr;
  long len;
};
inline void snap_sort(std::vector<SnapRange>& r) {   // insertion sort: a few hundred leaves at the most, and no <algorithm> needed
  for (size_t i = 1; i < r.size(); ++i) {
    const SnapRange x = r[i];
    size_t j = i;
    for (; j > 0 && r[j - 1].addr > x.addr; --j) r[j] = r[j - 1];
    r[j] = x;
  }
}
inline std::vector<SnapRange> snap_merge(std::vector<SnapRange> r) {
  snap_sort(r);
  std::vector<SnapRange> out;
  for (const SnapRange& x : r) {
    if (x.len <= 0) continue;
    if (!out.empty() && out.back().addr + (uintptr_t)out.back().len * sizeof(float) == x.addr) out.back().len += x.len;
    else out.push_back(x);
  }
  return out;
}

}  // namespace serl
