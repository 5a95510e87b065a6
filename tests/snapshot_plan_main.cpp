// Proof of serl_amd/csrc/snapshot_plan.h on the CPU (tests/test_snapshot_plan_cpu.py builds this with the host address and
// undefined-behaviour sanitizers).  For a list of cases -- run lengths of 1, 3, 4, 5, 4095, 4096, 4097 and 3*4096+2 floats, several
// runs per section, empty sections -- it checks that the parts tile every run exactly once, that every vector body is 16-byte
// aligned in source and destination, that tails are shorter than four floats and sit at the end of their run, that section tags
// are right and that the staging size is the header plus the runs rounded up to 16 bytes.  Then a host model of
// snapshot_pack_kernel moves real floats part by part (body as whole 16-byte vectors, tail one by one, counting exponent-all-ones
// values per section) from sources placed at 16-byte aligned addresses into a staging buffer whose padding is poisoned: every run
// must arrive intact, no byte outside a run may change, and the counts must match what was planted.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "snapshot_plan.h"

using namespace serl;

#define CHECK(c, ...)                        \
  do {                                       \
    if (!(c)) {                              \
      std::printf("FAILED %s: ", #c);        \
      std::printf(__VA_ARGS__);              \
      std::printf("\n");                     \
      std::exit(1);                          \
    }                                        \
  } while (0)

static bool nonfinite(float x) {
  uint32_t u;
  std::memcpy(&u, &x, 4);
  return (u & 0x7f800000u) == 0x7f800000u;
}

static void run_case(const char* name, const std::vector<SnapRun>& runs) {
  const SnapPlan p = snapshot_plan(runs);
  // ---- the layout
  size_t want_bytes = kSnapHeaderBytes;
  CHECK(p.run_dst.size() == runs.size(), "%s", name);
  for (size_t r = 0; r < runs.size(); ++r) {
    CHECK(p.run_dst[r] == want_bytes && p.run_dst[r] % 16 == 0, "%s run %zu at %zu", name, r, p.run_dst[r]);
    want_bytes += ((size_t)runs[r].len * 4 + 15) / 16 * 16;
  }
  CHECK(p.bytes == want_bytes, "%s: %zu bytes, expected %zu", name, p.bytes, want_bytes);
  // ---- the parts tile every run exactly once
  std::vector<std::vector<int>> seen(runs.size());
  for (size_t r = 0; r < runs.size(); ++r) seen[r].assign((size_t)runs[r].len, 0);
  long expected_parts = 0;
  for (const SnapRun& r : runs) expected_parts += (r.len + kSnapPartFloats - 1) / kSnapPartFloats;
  CHECK((long)p.parts.size() == expected_parts, "%s: %zu parts, expected %ld", name, p.parts.size(), expected_parts);
  for (const SnapPart& q : p.parts) {
    CHECK(q.run >= 0 && q.run < (int)runs.size(), "%s", name);
    const SnapRun& r = runs[q.run];
    CHECK(q.section == r.section, "%s: part of run %d tagged %d, run is section %d", name, q.run, q.section, r.section);
    CHECK(q.len >= 1 && q.len <= kSnapPartFloats && q.off >= 0 && q.off + q.len <= r.len, "%s: part [%ld, +%d) of a run of %ld", name, q.off, q.len, r.len);
    CHECK(q.body % 4 == 0 && q.body + q.tail == q.len && q.tail >= 0 && q.tail < 4, "%s: body %d tail %d len %d", name, q.body, q.tail, q.len);
    CHECK(q.tail == 0 || q.off + q.len == r.len, "%s: a tail inside a run", name);
    CHECK((q.off * 4) % 16 == 0 && q.dst % 16 == 0, "%s: body not 16-byte aligned (source offset %ld floats, destination %zu)", name, q.off, q.dst);
    CHECK(q.dst == p.run_dst[q.run] + (size_t)q.off * 4, "%s", name);
    for (int i = 0; i < q.len; ++i) seen[q.run][(size_t)q.off + i] += 1;
  }
  for (size_t r = 0; r < runs.size(); ++r)
    for (long i = 0; i < runs[r].len; ++i) CHECK(seen[r][(size_t)i] == 1, "%s: float %ld of run %zu covered %d times", name, i, r, seen[r][(size_t)i]);
  // ---- a host model of the kernel on real memory
  std::vector<float*> src(runs.size());
  long planted[kSnapSections] = {0, 0, 0};
  const float specials[] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(),
                            1e-42f /* denormal */, -0.0f, 3.4e38f};
  for (size_t r = 0; r < runs.size(); ++r) {
    src[r] = static_cast<float*>(std::aligned_alloc(16, ((size_t)runs[r].len * 4 + 15) / 16 * 16));
    for (long i = 0; i < runs[r].len; ++i) src[r][i] = (float)(r * 100003 + i) * 0.25f;
    // first, last (the tail path) and a middle element get special values; only NaN and the Infs count
    const long at[3] = {0, runs[r].len - 1, runs[r].len / 2};
    for (int k = 0; k < 3; ++k) src[r][at[k]] = specials[(r * 3 + k) % 6];
    for (long i = 0; i < runs[r].len; ++i) planted[runs[r].section] += nonfinite(src[r][i]);
  }
  std::vector<uint8_t> slot(p.bytes, 0xAB);
  uint32_t counters[kSnapSections] = {0, 0, 0};
  for (const SnapPart& q : p.parts) {
    const float* s = src[q.run] + q.off;
    uint8_t* d = slot.data() + q.dst;
    CHECK(reinterpret_cast<uintptr_t>(s) % 16 == 0, "%s: source of a body at %p", name, (const void*)s);
    for (int v = 0; v < q.body / 4; ++v) {
      float x[4];
      std::memcpy(x, s + 4 * v, 16);
      for (float e : x) counters[q.section] += nonfinite(e);
      std::memcpy(d + 16 * v, x, 16);
    }
    for (int t = 0; t < q.tail; ++t) {
      counters[q.section] += nonfinite(s[q.body + t]);
      std::memcpy(d + 4 * (q.body + t), s + q.body + t, 4);
    }
  }
  std::vector<uint8_t> want(p.bytes, 0xAB);
  for (size_t r = 0; r < runs.size(); ++r) std::memcpy(want.data() + p.run_dst[r], src[r], (size_t)runs[r].len * 4);
  CHECK(std::memcmp(want.data(), slot.data(), p.bytes) == 0, "%s: the staging slot differs from the runs laid out back to back", name);
  for (int s = 0; s < kSnapSections; ++s) CHECK((long)counters[s] == planted[s], "%s: section %d counted %u, planted %ld", name, s, counters[s], planted[s]);
  for (float* s : src) std::free(s);
  std::printf("case %s runs=%zu parts=%zu bytes=%zu nonfinite=%u,%u,%u\n", name, runs.size(), p.parts.size(), p.bytes, counters[0], counters[1], counters[2]);
}

int main() {
  const long lens[] = {1, 3, 4, 5, 4095, 4096, 4097, 3 * 4096 + 2};
  char name[64];
  for (long n : lens) {
    std::snprintf(name, sizeof(name), "single_%ld", n);
    run_case(name, {{n, 0}});
  }
  run_case("empty", {});
  run_case("all_lengths_one_section", {{1, 1}, {3, 1}, {4, 1}, {5, 1}, {4095, 1}, {4096, 1}, {4097, 1}, {3 * 4096 + 2, 1}});
  run_case("several_runs_per_section", {{5, 0}, {4097, 0}, {3, 1}, {4096, 1}, {1, 2}, {4095, 2}, {3 * 4096 + 2, 2}, {1, 2}});
  run_case("empty_middle_section", {{4097, 0}, {1, 0}, {3 * 4096 + 2, 2}, {3, 2}});
  run_case("only_last_section", {{5, 2}, {4, 2}});
  // snap_merge: ranges given out of order, two of them touching, one apart
  std::vector<SnapRange> r = {{4096 + 40, 6}, {4096, 10}, {8192, 4}};
  const std::vector<SnapRange> m = snap_merge(r);
  CHECK(m.size() == 2 && m[0].addr == 4096 && m[0].len == 16 && m[1].addr == 8192 && m[1].len == 4, "snap_merge");
  std::printf("ok\n");
  return 0;
}
