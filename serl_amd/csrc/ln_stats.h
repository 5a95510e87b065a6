// The row statistics of the one-wave-per-row LayerNorm kernels (heads.hip, classifier.hip).  Device code only.
#pragma once
#include <hip/hip_runtime.h>

namespace serl {

// s1 and s2 summed over the 64 lanes of the wave, the sums left in every lane (xor butterfly)
__device__ __forceinline__ void wave_sum2(float& s1, float& s2) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) { s1 += __shfl_xor(s1, off); s2 += __shfl_xor(s2, off); }
}

// mean and 1 / sqrt(var + 1e-6) of a row of D values from their sum s1 and their sum of squares s2 (fast variance, clamped at 0)
template <int D>
__device__ __forceinline__ void ln_mean_rstd(float s1, float s2, float& mean, float& rstd) {
  mean = s1 * (1.0f / D);
  const float mean2 = s2 * (1.0f / D);
  const float var = fmaxf(mean2 - mean * mean, 0.f);
  rstd = rsqrtf(var + 1e-6f);
}

// ... of a row whose `d` live values lie in a wider, zero-padded row: the pads add nothing to s1 and s2, the divisor is d
__device__ __forceinline__ void ln_mean_rstd_n(float s1, float s2, int d, float& mean, float& rstd) {
  const float inv = 1.0f / (float)d;
  mean = s1 * inv;
  const float mean2 = s2 * inv;
  const float var = fmaxf(mean2 - mean * mean, 0.f);
  rstd = rsqrtf(var + 1e-6f);
}

}  // namespace serl
