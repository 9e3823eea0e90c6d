// The random stream of sampled decoding (vocab_sample.hip, capnet_sample_uniform), host and device.
//   sample_uniform(seed, step, row, v): a pure function of its four integers --
//     c = (step << 48) | (row << 24) | v        injective for step <= 65535, row < 2^24, v < 2^24
//     z = seed + 0x9E3779B97F4A7C15 (c + 1)     (mod 2^64), then dropout_mask.h's three-line finalizer
//     b = z >> 41                               23 bits
//     u = (2 b + 1) / 2^24                      an odd multiple of 2^-24: exact in fp32, 2^-24 <= u <= 1 - 2^-24
//   so 0 and 1 are impossible and sample_gumbel(u) = -logf(-logf(u)) is finite, within [-2.82, 16.64]. The stream has
//   2^23 distinct values per draw.
//   argmax_v (logit_v / T + sample_gumbel(u_v)) is a draw from softmax(logit / T) (Gumbel-max): every kernel that samples
//   adds this noise keyed by (seed, step, row, vocabulary index), so the draw does not depend on how the vocabulary is
//   split over workgroups, launches or candidate lists.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace capnet {

__host__ __device__ __forceinline__ float sample_uniform(unsigned long long seed, unsigned step, unsigned row, unsigned v) {
  const unsigned long long c = ((unsigned long long)step << 48) | ((unsigned long long)row << 24) | (unsigned long long)v;
  unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (c + 1ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  const unsigned b = (unsigned)(z >> 41);
  return (float)(2u * b + 1u) * (1.0f / 16777216.0f);
}

// full-precision logf, not the fast intrinsic: the tests bound this function's error (TOL_G)
__host__ __device__ __forceinline__ float sample_gumbel(float u) { return -logf(-logf(u)); }

}  // namespace capnet
