// Exclusions as a bit mask: what a row may not draw -- or, in the fused beam step, may not select -- at a
// step, for the vocabulary kernels' epilogues to read.
//   mask [rows][W] of 32-bit words, W = ceil(V / 32): bit v & 31 of word v >> 5 of row r is set where word v is excluded on
//   launch row r at this step. kVocCols is 32, so workgroup b of the vocabulary kernels needs exactly word b of every row.
// exclusion_mask_kernel<T>: capnet.beam.banned_words at step `step` on the hypothesis [start[r], words[r][0 .. m)] (start
// null: the words alone), ONE kernel over both token sources --
//   the sampler's (sample_exclusion_mask): T = int64, words = the caller's ids matrix, m = t drawn words, <start> beside
//     them, step = t + 1, the tokens as drawn whether or not the row has emitted <end>;
//   the beam state's (beam_exclusion_mask): T = int32, words = the rows of BeamState.seq[(step - 1) & 1] (row stride
//     max_steps + 2), m = step tokens with <start> already first, no start array -- the tokens BeamExclState reads.
// The rule: every word of `banned`; <end> while step <= min_words; g = no_repeat_ngram >= 1 and n >= g tokens: for every
//   start position e of a g-gram whose first g - 1 tokens equal the hypothesis' last g - 1, the token behind them (g = 1:
//   every token; a context seen several times excludes several words). A word outside [0, V) is never an address (the rows
//   of dead beam slots hold stale tokens; their masks are never read).
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

template <class T>
__global__ __launch_bounds__(kMaskThreads) void exclusion_mask_kernel(
    const T* __restrict__ ids, long ld, const long long* __restrict__ start, int m, int step, int V, int W, long long end_token,
    int g, int min_words, const int* __restrict__ banned, int n_banned, unsigned* __restrict__ mask) {
  __shared__ unsigned bits[kMaskChunk];
  const int row = blockIdx.x, tid = threadIdx.x;
  const T* words = ids + (long)row * ld;             // read at 0 .. m - 1 only
  const int lead = start ? 1 : 0, n = m + lead;
  // <start> is read ONCE, here, behind a branch the whole workgroup takes alike. Read inside tok() its address is uniform but
  // its condition is per thread, and the compiler then issues the load as a scalar load in a block it enters with an empty
  // exec mask too: with start null that is a load from address 8 row.
  const long long first = start ? start[row] : 0;
  auto tok = [&](int i) -> long long { return i < lead ? first : (long long)words[i - lead]; };
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
  hipLaunchKernelGGL(exclusion_mask_kernel<long long>, dim3(rows), dim3(kMaskThreads), 0, stream, ids, ld, start_tokens, t, t + 1,
                     V, sample_mask_words(V), c.end_token, c.no_repeat_ngram, c.min_words, c.banned, c.n_banned, mask);
  CAPNET_LAUNCH_CHECK();
  return kOk;
}

// the same kernel on the hypotheses a device beam search keeps: row r of the mask is row r of the decode step (image r / k,
// slot r % k), its `step` tokens those of BeamState.seq[(step - 1) & 1]
int beam_exclusion_mask(const void* beam, int n, int k, int max_steps, int step, int V, long long end_token,
                        const BeamConstraints& c, unsigned* mask, hipStream_t stream) {
  CAPNET_REQUIRE(beam && mask && n >= 1 && k >= 1 && (long)n * k < (1L << 24) && V >= 1 && V <= (1 << 24) && step >= 1 &&
                     step <= max_steps,
                 "beam_exclusion_mask: n %d, k %d, V %d, step %d of %d", n, k, V, step, max_steps);
  const int* tokens = nullptr;
  if (int rc = beam_tokens(beam, n, k, max_steps, step, &tokens)) return rc;
  hipLaunchKernelGGL(exclusion_mask_kernel<int>, dim3(n * k), dim3(kMaskThreads), 0, stream, tokens, (long)(max_steps + 2),
                     (const long long*)nullptr, step, step, V, sample_mask_words(V), end_token, c.no_repeat_ngram, c.min_words,
                     c.banned, c.n_banned, mask);
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
