// The scaled logit and the Gumbel-max key of sampled decoding, formed the same way by every kernel that samples
// (vocab_sample.hip, vocab_nucleus.hip). Include it after the other headers.
#pragma once
#include "sample_rng.h"

// No contraction into fused multiply-adds from here to the end of the including file: s = z inv_T is a rounded product
// wherever it is formed, so every kernel forms the same key bits from the same logit, expf(s - M) of the largest s is exactly
// 1 and a single candidate's logp is exactly 0 (hipcc contracts across statements by default, and __fmul_rn is a plain
// product to it).
#pragma clang fp contract(off)

namespace capnet {

// the key of entry v of noise row `nrow`: separate roundings of the product and of the sum (see the pragma above)
__device__ __forceinline__ float vs_scaled(float z, float inv_T) { return __fmul_rn(z, inv_T); }
__device__ __forceinline__ float vs_key(float s, unsigned long long seed, unsigned step, unsigned nrow, unsigned v) {
  return __fadd_rn(s, sample_gumbel(sample_uniform(seed, step, nrow, v)));
}

}  // namespace capnet
