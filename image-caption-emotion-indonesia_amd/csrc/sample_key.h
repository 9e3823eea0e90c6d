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

// The key of entry v of PHYSICAL row `prow` of a decode that carries greedy rows -- the one place that knows their layout.
// greedy_stride 0: no greedy rows, the noise row is the physical row (the bits of vs_key(s, seed, step, prow, v)).
// greedy_stride g >= 1: the rows come in groups of g (an image's), the first g - 1 drawn and the last one greedy:
//   row i g + j, j < g - 1, is sample j of image i and takes noise row i (g - 1) + j -- the row it has in the same decode
//   without greedy rows, so its draws are the same;
//   row i g + g - 1 is the greedy row: its key is s itself (Gumbel-max with the noise switched off is the argmax; the
//   total order of vocab_better then sends ties to the lower index).
__device__ __forceinline__ float vs_row_key(float s, unsigned long long seed, unsigned step, unsigned prow, unsigned greedy_stride,
                                            unsigned v) {
  if (greedy_stride == 0) return vs_key(s, seed, step, prow, v);
  const unsigned i = prow / greedy_stride, j = prow - i * greedy_stride;
  if (j == greedy_stride - 1) return s;
  return vs_key(s, seed, step, i * (greedy_stride - 1) + j, v);
}

}  // namespace capnet
