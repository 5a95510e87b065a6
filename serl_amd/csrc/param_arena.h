// Host-side plumbing of the handles' device arenas (agent.hip, bc.hip, classifier.hip): the leaf table of a flat parameter
// vector, the 256-byte bump carve of an arena, allocating it, and the host <-> device copy of one leaf.
#pragma once
#include <string>
#include <vector>

#include "common.h"

namespace serl {

// A named slice [off, off + count) of a flat float parameter vector.
struct Leaf {
  std::string name;
  long off, count;
};

// Appends a leaf of `count` floats at `off` and moves `off` behind it; returns the leaf's offset.
inline long add_leaf(std::vector<Leaf>& v, long& off, std::string name, long count) {
  v.push_back({std::move(name), off, count});
  off += count;
  return off - count;
}

inline const Leaf* find(const std::vector<Leaf>& v, const char* name) {
  for (const Leaf& l : v)
    if (l.name == name) return &l;
  return nullptr;
}

inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

// Carves consecutive 256-byte aligned pieces out of an arena; with base == nullptr it only measures (off = total bytes).
struct Bump {
  uint8_t* base;
  size_t off = 0;
  explicit Bump(void* b) : base((uint8_t*)b) {}
  template <typename T>
  T* take(size_t n) {
    T* p = base ? (T*)(base + off) : nullptr;
    off += al256(n * sizeof(T));
    return p;
  }
};

// K-split of a GEMM launch: the deepest power-of-two split up to `smax` that keeps the launch within `budget` workgroups.
inline int split_under(int M, int N, int groups, int smax, long budget = 512) {
  const long tiles = (long)cdiv(M, 64) * cdiv(N, 64) * groups;
  int s = smax;
  while (s > 1 && tiles * s > budget) s >>= 1;
  return s;
}

// hipMalloc + zero-fill of an arena of `bytes`; on failure *out is untouched and the error is set.
inline int alloc_zeroed(void** out, size_t bytes, const char* what) {
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, bytes);
  if (e != hipSuccess) {
    set_error("hipMalloc of %zu bytes for the %s failed: %s", bytes, what, hipGetErrorString(e));
    return SERL_ERR_HIP;
  }
  e = hipMemset(p, 0, bytes);
  if (e != hipSuccess) {
    (void)hipFree(p);
    set_error("hipMemset of the %s failed: %s", what, hipGetErrorString(e));
    return SERL_ERR_HIP;
  }
  *out = p;
  return SERL_OK;
}

// Copies the n floats of a leaf between the host and the device (`kind`: which way).  A nullptr device side is an Adam moment
// that is zero by construction (a frozen leaf's, or one outside its optimizer's support): it reads as zeros, and what is written
// to it must be all zeros -- else the error `nonzero_fmt`, formatted with the section and the leaf name.
inline int leaf_copy(float* dst, const float* src, long n, hipMemcpyKind kind, const char* section, const char* leaf,
                     const char* nonzero_fmt) {
  if (kind == hipMemcpyHostToDevice && !dst) {
    for (long i = 0; i < n; ++i) SERL_REQUIRE(src[i] == 0.f, nonzero_fmt, section, leaf);
    return SERL_OK;
  }
  if (kind == hipMemcpyDeviceToHost && !src) {
    for (long i = 0; i < n; ++i) dst[i] = 0.f;
    return SERL_OK;
  }
  SERL_HIP(hipMemcpy(dst, src, (size_t)n * sizeof(float), kind));
  return SERL_OK;
}

}  // namespace serl
