// Host-side plumbing of the handles' device arenas (agent.hip, bc.hip, classifier.hip): the leaf table of a flat parameter
// vector, the 256-byte bump carve of an arena, allocating it, and the host <-> device copy of one leaf.
#pragma once
#include <string>
#include <vector>

#include "common.h"

namespace serl {

// A named slice of a flat float parameter vector that starts at `off`.  `count` is the number of the leaf's own elements.  Most
// leaves are the contiguous [off, off + count).  A BOX leaf (a ragged MLP layer) is `n` blocks of `rows` x
// `cols` elements stored inside n blocks of rows_p x ld floats: element (i, r, c) lies at off + (i * rows_p + r) * ld + c, and the
// floats of the storage outside the box are padding that is zero and stays zero.  span() is the storage, what `off` advances by.
struct Leaf {
  std::string name;
  long off, count;
  long n = 1, rows = 1, cols = 0, rows_p = 1, ld = 0;   // cols == 0: contiguous, the box fields say nothing
  // whether a copy of the leaf has to be strided: padding BEHIND the last row of a one-block leaf (rows_p > rows with ld == cols)
  // leaves the leaf's elements one contiguous run; span() != count is the test for "has padding"
  bool boxed() const { return cols != 0 && (ld != cols || (n > 1 && rows_p != rows)); }
  long span() const { return cols == 0 ? count : n * rows_p * ld; }
};

// Appends a leaf of `count` floats at `off` and moves `off` behind it; returns the leaf's offset.
inline long add_leaf(std::vector<Leaf>& v, long& off, std::string name, long count) {
  v.push_back({std::move(name), off, count});
  off += count;
  return off - count;
}

// Appends a box leaf (Leaf, above) and moves `off` behind its storage; returns the leaf's offset.
inline long add_leaf_box(std::vector<Leaf>& v, long& off, std::string name, long n, long rows, long cols, long rows_p, long ld) {
  Leaf l{std::move(name), off, n * rows * cols};
  l.n = n; l.rows = rows; l.cols = cols; l.rows_p = rows_p; l.ld = ld;
  v.push_back(l);
  off += l.span();
  return l.off;
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

// ... of a leaf `l` whose device side `dev` (nullptr: as above) may be a box: the host side is the leaf's count elements, dense,
// in (block, row, column) order; the padding of the storage is neither read nor written.
inline int leaf_copy(float* dev, float* host_out, const float* host_in, const Leaf& l, hipMemcpyKind kind, const char* section,
                     const char* nonzero_fmt) {
  const bool up = kind == hipMemcpyHostToDevice;
  if (!dev || !l.boxed())
    return up ? leaf_copy(dev, host_in, l.count, kind, section, l.name.c_str(), nonzero_fmt)
              : leaf_copy(host_out, dev, l.count, kind, section, l.name.c_str(), nonzero_fmt);
  for (long i = 0; i < l.n; ++i) {
    float* d = dev + i * l.rows_p * l.ld;
    const long h = i * l.rows * l.cols;
    if (up) SERL_HIP(hipMemcpy2D(d, l.ld * sizeof(float), host_in + h, l.cols * sizeof(float), l.cols * sizeof(float), l.rows, kind));
    else SERL_HIP(hipMemcpy2D(host_out + h, l.cols * sizeof(float), d, l.ld * sizeof(float), l.cols * sizeof(float), l.rows, kind));
  }
  return SERL_OK;
}

}  // namespace serl
