// The dropout mask of the decoders (input embeddings and the rows between stacked layers), shared by every kernel that
// draws or re-draws it.
#pragma once
#include <hip/hip_runtime.h>

namespace capnet {

// counter-based dropout mask: keep iff u(seed, sample, col, e) >= p. Recomputed in backward.
__device__ __forceinline__ float dropout_scale(unsigned long long seed, int sample, int col, int e,
                                               float p, float inv_keep) {
  unsigned long long z = seed + 0x9E3779B97F4A7C15ull *
                                    ((((unsigned long long)(unsigned)sample << 20) ^
                                      ((unsigned long long)(unsigned)col << 10)) *
                                         1000003ull +
                                     (unsigned long long)(unsigned)e + 1ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  const float u = (float)(z >> 40) * (1.0f / 16777216.0f);
  return u >= p ? inv_keep : 0.f;
}

}  // namespace capnet
