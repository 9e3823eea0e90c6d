// Sampled decoding with exclusions: what a row may not draw at a step, as a bit mask the draws read.
//   mask [rows][W] of 32-bit words, W = ceil(V / 32): bit v & 31 of word v >> 5 of row r is set where word v is excluded on
//   launch row r at this step. kVocCols is 32, so workgroup b of the vocabulary kernels needs exactly word b of every row.
// sample_exclusion_mask_kernel: the mask of stream step t (0-based) from what is on the device -- capnet.beam.banned_words
// on the hypothesis [start[r], ids[r][0] .. ids[r][t - 1]] at step t + 1 (start null: the words alone), the tokens as drawn
// whether or not the row has emitted <end>:
//   every word of `banned`; <end> while t + 1 <= min_words; g = no_repeat_ngram >= 1 and n >= g tokens: for every start
//   position e of a g-gram whose first g - 1 tokens equal the hypothesis' last g - 1, the token behind them (g = 1: every
//   token; a context seen several times excludes several words). A word outside [0, V) is never an address.
// One workgroup per row. The row's mask is built in LDS a chunk of kMaskChunk words at a time (one chunk up to V = 65536):
// zero, LDS atomic OR per excluded word of the chunk, vector stores of the whole chunk -- every word of the row is written,
// so the mask needs no clearing between steps.
// mask_logits_kernel: -inf at the mask's set bits of a [rows][ld] logits block, for the draws that read their logits from
// memory (sample_rows, nucleus_rows, torch.topk in front of the picks): they treat -inf as not pickable.
#include "common.h"
#include "kernels.h"

namespace capnet {

constexpr int kMaskThreads = 256;
constexpr int kMaskChunk = 2048;      // mask words per pass: 8 KB of LDS

__global__ __launch_bounds__(kMaskThreads) void sample_exclusion_mask_kernel(
    const long long* __restrict__ ids, long ld, const long long* __restrict__ start, int t, int V, int W, long long end_token,
    int g, int min_words, const int* __restrict__ banned, int n_banned, unsigned* __restrict__ mask) {
  __shared__ unsigned bits[kMaskChunk];
  const int row = blockIdx.x, tid = threadIdx.x;
  const long long* words = ids + (long)row * ld;     // read at 0 .. t - 1 only
  const int lead = start ? 1 : 0, n = t + lead, step = t + 1;
  auto tok = [&](int i) -> long long { return i < lead ? start[row] : words[i - lead]; };
  unsigned* out = mask + (long)row * W;
  for (int c0 = 0; c0 < W; c0 += kMaskChunk) {
    const int cw = min(kMaskChunk, W - c0);
    for (int j = tid; j < cw; j += kMaskThreads) bits[j] = 0u;
    __syncthreads();
    auto put = [&](long long w) {
      if (w < 0 || w >= V) return;
      const int at = (int)(w >> 5) - c0;
      if (at >= 0 && at < cw) atomicOr(&bits[at], 1u << (unsigned)(w & 31));
    };
    for (int q = tid; q <= n_banned; q += kMaskThreads)
      put(q < n_banned ? (long long)banned[q] : step <= min_words ? end_token : -1);
    if (g >= 1 && n >= g) {
      const int starts = n - g + 1;
      for (int e = tid; e < starts; e += kMaskThreads) {
        bool same = true;
        for (int c = 0; c < g - 1; ++c) same &= tok(e + c) == tok(n - (g - 1) + c);
        if (same) put(tok(e + g - 1));
      }
    }
    __syncthreads();
    for (int j = tid; j < cw; j += kMaskThreads) out[c0 + j] = bits[j];
    __syncthreads();   // bits is cleared by the next pass
  }
}

// thread (row, mask word j): the word's set bits, lowest first
__global__ __launch_bounds__(kMaskThreads) void mask_logits_kernel(float* __restrict__ logits, long ld, int V, int W,
                                                                   const unsigned* __restrict__ mask) {
  const int row = blockIdx.x, j = blockIdx.y * kMaskThreads + threadIdx.x;
  if (j >= W) return;
  unsigned m = mask[(long)row * W + j];
  float* x = logits + (long)row * ld + 32L * j;
  while (m) {
    const int b = __ffs(m) - 1;
    m &= m - 1;
    if (32 * j + b < V) x[b] = -INFINITY;
  }
}

size_t sample_mask_bytes(int rows, int V) { return align16((size_t)rows * sample_mask_words(V) * sizeof(unsigned)); }

int sample_excl_check(const char* who, const SampleExcl& c) {
  CAPNET_REQUIRE(c.no_repeat_ngram >= 0 && c.no_repeat_ngram <= 4, "%s: no_repeat_ngram=%d (0 .. 4)", who, c.no_repeat_ngram);
  CAPNET_REQUIRE(c.min_words >= 0, "%s: min_words=%d (>= 0)", who, c.min_words);
  CAPNET_REQUIRE(c.n_banned >= 0 && c.n_banned <= 32, "%s: n_banned=%d (0 .. 32)", who, c.n_banned);
  CAPNET_REQUIRE((c.banned || !c.n_banned) && (size_t)c.banned % 4 == 0, "%s: banned must be a 4-byte aligned device array", who);
  return kOk;
}

int sample_exclusion_mask(const long long* ids, long ld, const long long* start_tokens, int rows, int t, int V,
                          const SampleExcl& c, unsigned* mask, hipStream_t stream) {
  CAPNET_REQUIRE(rows >= 1 && rows < (1 << 24) && V >= 1 && V <= (1 << 24) && t >= 0 && (ids || !t) && mask,
                 "sample_exclusion_mask: rows %d, V %d, t %d", rows, V, t);
  hipLaunchKernelGGL(sample_exclusion_mask_kernel, dim3(rows), dim3(kMaskThreads), 0, stream, ids, ld, start_tokens, t, V,
                     sample_mask_words(V), c.end_token, c.no_repeat_ngram, c.min_words, c.banned, c.n_banned, mask);
  CAPNET_LAUNCH_CHECK();
  return kOk;
}

int mask_logits(float* logits, int rows, long ld, int V, const unsigned* mask, hipStream_t stream) {
  CAPNET_REQUIRE(rows >= 1 && rows < (1 << 24) && V >= 1 && V <= (1 << 24) && ld >= V && logits && mask, "mask_logits: rows %d, V %d, ld %ld", rows, V, ld);
  const int W = sample_mask_words(V);
  hipLaunchKernelGGL(mask_logits_kernel, dim3(rows, (W + kMaskThreads - 1) / kMaskThreads), dim3(kMaskThreads), 0, stream, logits,
                     ld, V, W, mask);
  CAPNET_LAUNCH_CHECK();
  return kOk;
}

}  // namespace capnet
