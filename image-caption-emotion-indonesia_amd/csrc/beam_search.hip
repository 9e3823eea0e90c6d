// The selection step of beam search (capnet.beam, the one-call searches of decode_loops.hip): the functors a step's
// selection is built from -- exclusions (constraints), the Hamming penalty (diverse teams), the forced-word pool -- and
// beam_topk_body, which runs them around log-softmax + running score + top-k; the kernels of the host loops' form
// (beam_topk[_batched][_banned | _diverse | _forced]); and the search whose bookkeeping stays on the device: the state
// and its trace, beam_init, the beam_advance kernels with their shared tail, beam_advance_topk, beam_finish, beam_nbest.
#include "common.h"
#include "kernels.h"

namespace capnet {

// ---- beam-search expansion: log-softmax + running score + top-k over rows*V ------------------
// One launch per decode step of sample() (stylenet/model.py:233-249): scores[r][v] =
// prev[r] + log_softmax(logits[r])[v]; the k best of the flattened [rows*V] array, best first,
// ties to the lower flat index. One workgroup: rows <= 16 beams x V is a few hundred KB.
constexpr int kBeamThreads = 1024, kBeamMax = 16;

__device__ __forceinline__ void beam_better(float v, long i, float& bv, long& bi) {
  if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
}

// ---- constrained search: what a step must not select. An exclusion is a functor beam_topk_body runs AFTER the
// rows' log-sum-exp (taken over the whole, unmodified rows) and BEFORE the k selection passes: it writes -INFINITY over
// the excluded entries of the logits block itself -- the step's scratch, recomputed next step on every route -- so the
// selection needs no second list to consult and the survivors' scores are the model's own log-probabilities. kActive
// false: no code at all, and the logits stay const __restrict__ (the unconstrained kernels compile to what they were).
constexpr int kBanMax = 32, kNgramMax = 4;
typedef const float* __restrict__ beam_logits_ro;

struct BeamNoExcl {
  typedef beam_logits_ro logits_t;
  static constexpr bool kActive = false;
  __device__ __forceinline__ void operator()(logits_t, long, int, int) const {}
};

// the exclusions of the device routes, derived from the image's own hypotheses: tok = the image's rows of
// BeamState.seq[(step - 1) & 1] ([k][L], `step` tokens each, <start> first). banned words on every row; <end> while step <=
// min_words; g = no_repeat_ngram >= 1 and step >= g: a thread per (row, start position e), g - 1 compares -- the g - 1
// words at e against the row's last g - 1 -- and where they agree the word behind them goes. Several threads may write the
// same -INFINITY. A word outside [0, V) is never an address.
struct BeamExclState {
  typedef float* logits_t;
  static constexpr bool kActive = true;
  const int* tok;
  int L, step, g, min_words;
  long long end_token;
  const int* banned;
  int n_banned;
  __device__ __forceinline__ void operator()(float* logits, long ld, int rows, int V) const {
    const int tid = threadIdx.x, fixed = n_banned + 1;
    for (int t = tid; t < rows * fixed; t += kBeamThreads) {
      const int r = t / fixed, q = t % fixed;
      const long long w = q < n_banned ? (long long)banned[q] : step <= min_words ? end_token : -1;
      if (w >= 0 && w < V) logits[(long)r * ld + w] = -INFINITY;
    }
    if (g >= 1 && step >= g) {
      const int starts = step - g + 1;
      for (int t = tid; t < rows * starts; t += kBeamThreads) {
        const int r = t / starts, e = t % starts;
        const int* q = tok + (long)r * L;
        bool same = true;
        for (int c = 0; c < g - 1; ++c) same &= q[e + c] == q[step - (g - 1) + c];
        const int w = q[e + g - 1];
        if (same && w >= 0 && w < V) logits[(long)r * ld + w] = -INFINITY;
      }
    }
  }
};

// the exclusions of the host routes, which hold the sequences in Python (capnet.beam.banned_words): bans int32
// [rows][1 + cap], per row of the logits its count, then that many words
struct BeamExclList {
  typedef float* logits_t;
  static constexpr bool kActive = true;
  const int* bans;
  int cap;
  __device__ __forceinline__ void operator()(float* logits, long ld, int rows, int V) const {
    for (int t = threadIdx.x; t < rows * cap; t += kBeamThreads) {
      const int r = t / cap, q = t % cap;
      const int* b = bans + (long)r * (1 + cap);
      const int w = b[1 + q];
      if (q < b[0] && w >= 0 && w < V) logits[(long)r * ld + w] = -INFINITY;
    }
  }
};

// the exclusions of the diverse host route: BeamExclList, or nothing where bans is null
struct BeamExclListOrNone {
  typedef float* logits_t;
  static constexpr bool kActive = true;
  const int* bans;
  int cap;
  __device__ __forceinline__ void operator()(float* logits, long ld, int rows, int V) const {
    if (bans) BeamExclList{bans, cap}(logits, ld, rows, V);
  }
};

// ---- diverse search: the Hamming penalty of a later team. A penalty is a second functor beam_topk_body
// runs after the exclusions: apply() writes logit - strength * count over the listed words of every competing row (at
// most kBeamMax (word, count) pairs, the words distinct, so no two threads share an address) after saving the originals
// in LDS; the selection passes then rank by the penalised key without consulting anything. score() gives back what is
// carried forward and reported: (prev - lse) + the ORIGINAL logit, formed exactly as the plain selection forms it. At
// strength 0 the key is the score bit for bit. kActive false: no code at all.
struct BeamNoPen {
  static constexpr bool kActive = false;
};

struct BeamPenList {
  static constexpr bool kActive = true;
  const int *word, *count;   // LDS, [kBeamMax]
  int n_words;
  float strength;
  float* orig;               // LDS, [kBeamMax rows][kBeamMax words]
  __device__ __forceinline__ void apply(float* logits, long ld, int rows, int V) const {
    for (int t = threadIdx.x; t < rows * n_words; t += kBeamThreads) {
      const int r = t / n_words, q = t % n_words, w = word[q];
      if (w >= 0 && w < V) {
        const float x = logits[(long)r * ld + w];
        orig[r * kBeamMax + q] = x;
        logits[(long)r * ld + w] = x - strength * (float)count[q];
      }
    }
  }
  __device__ __forceinline__ float score(const float* logits, long ld, int V, long flat, float base) const {
    const int r = (int)(flat / V), w = (int)(flat % V);
    float x = logits[(long)r * ld + w];
    for (int q = 0; q < n_words; ++q)
      if (word[q] == w) x = orig[r * kBeamMax + q];
    return base + x;
  }
};

// ---- forced words: what runs behind the k plain passes. A pool is a third functor of beam_topk_body: it is
// handed the rows' log-sum-exp and the plain selection (out_scores / out_index, which then lie in LDS) and replaces it
// with its own. kActive false: no code at all.
struct BeamNoPool {
  static constexpr bool kActive = false;
};

// the expansion of ONE image's beams (a whole workgroup)
template <class Excl, class Pen = BeamNoPen, class Pool = BeamNoPool>
__device__ __forceinline__ void beam_topk_body(typename Excl::logits_t logits, long ld, int rows, int V,
                                               const float* __restrict__ prev, int k, float* __restrict__ out_scores,
                                               long long* __restrict__ out_index, const Excl excl = Excl(),
                                               const Pen pen = Pen(), const Pool pool = Pool()) {
  __shared__ float s_red[kBeamThreads / 64];
  __shared__ long s_idx[kBeamThreads / 64];
  __shared__ float s_lse[kBeamMax];
  __shared__ long s_sel[kBeamMax];
  __shared__ float s_bcast;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int r = 0; r < rows; ++r) {
    const float* p = logits + (long)r * ld;
    float m = -INFINITY;
    for (int v = tid; v < V; v += kBeamThreads) m = fmaxf(m, p[v]);
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if (lane == 0) s_red[wave] = m;
    __syncthreads();
    if (tid == 0) {
      float mm = s_red[0];
      for (int w = 1; w < kBeamThreads / 64; ++w) mm = fmaxf(mm, s_red[w]);
      s_bcast = mm;
    }
    __syncthreads();
    m = s_bcast;
    float sum = 0.f;
    for (int v = tid; v < V; v += kBeamThreads) sum += expf(p[v] - m);
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    __syncthreads();
    if (lane == 0) s_red[wave] = sum;
    __syncthreads();
    if (tid == 0) {
      float t = 0.f;
      for (int w = 0; w < kBeamThreads / 64; ++w) t += s_red[w];
      s_lse[r] = m + logf(t);
    }
    __syncthreads();
  }
  if constexpr (Excl::kActive) {   // every row's log-sum-exp is taken: now the excluded words leave the selection
    excl(logits, ld, rows, V);
    __syncthreads();
  }
  if constexpr (Pen::kActive) {   // after the exclusions: -inf stays -inf
    pen.apply(logits, ld, rows, V);
    __syncthreads();
  }
  for (int j = 0; j < k; ++j) {
    float bv = -INFINITY;
    long bi = 0x7fffffffffffffffL;
    for (int r = 0; r < rows; ++r) {
      const float* p = logits + (long)r * ld;
      const float base = prev[r] - s_lse[r];
      for (int v = tid; v < V; v += kBeamThreads) {
        const long flat = (long)r * V + v;
        bool taken = false;
        for (int q = 0; q < j; ++q) taken |= s_sel[q] == flat;
        if (!taken) beam_better(base + p[v], flat, bv, bi);
      }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o);
      const long oi = __shfl_xor(bi, o);
      beam_better(ov, oi, bv, bi);
    }
    __syncthreads();
    if (lane == 0) { s_red[wave] = bv; s_idx[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
      float v = s_red[0];
      long i = s_idx[0];
      for (int w = 1; w < kBeamThreads / 64; ++w) beam_better(s_red[w], s_idx[w], v, i);
      s_sel[j] = i;
      if constexpr (Pen::kActive)   // the unpenalised score (i past the rows: nothing was comparable, as in the plain body)
        if (i / V < rows) v = pen.score(logits, ld, V, i, prev[i / V] - s_lse[i / V]);
      out_scores[j] = v;
      out_index[j] = i;
    }
    __syncthreads();
  }
  if constexpr (Pool::kActive) pool(logits, ld, rows, V, prev, s_lse, k, out_scores, out_index);
}

__global__ __launch_bounds__(kBeamThreads) void beam_topk_kernel(
    const float* __restrict__ logits, long ld, int rows, int V, const float* __restrict__ prev,
    int k, float* __restrict__ out_scores, long long* __restrict__ out_index) {
  beam_topk_body<BeamNoExcl>(logits, ld, rows, V, prev, k, out_scores, out_index);
}

// many images at once (the test-set evaluator, stylenet/evaluator.py:63-120, decodes a whole batch per step): workgroup
// i expands image i's beams -- rows meta[3 i] .. + meta[3 i + 1] of the logits, its meta[3 i + 2] best; flat indices are
// local to the image (row within the image * V + word); images with k = 0 (finished) are skipped
__global__ __launch_bounds__(kBeamThreads) void beam_topk_batched_kernel(
    const float* __restrict__ logits, long ld, int V, const float* __restrict__ prev, const int* __restrict__ meta,
    float* __restrict__ out_scores, long long* __restrict__ out_index) {
  const int row0 = meta[3 * blockIdx.x], rows = meta[3 * blockIdx.x + 1], k = meta[3 * blockIdx.x + 2];
  if (k <= 0 || rows <= 0) return;
  beam_topk_body<BeamNoExcl>(logits + (long)row0 * ld, ld, rows, V, prev + row0, k, out_scores + (long)blockIdx.x * kBeamMax,
                             out_index + (long)blockIdx.x * kBeamMax);
}

int beam_topk(const float* logits, long ld, int rows, int V, const float* prev, int k,
              float* out_scores, long long* out_index, hipStream_t stream) {
  CAPNET_REQUIRE(logits && prev && out_scores && out_index, "beam_topk: null argument");
  CAPNET_REQUIRE(rows >= 1 && rows <= kBeamMax && k >= 1 && k <= kBeamMax && V >= 1 && ld >= V &&
                     (long)rows * V >= k,
                 "beam_topk: rows=%d k=%d V=%d (rows, k <= %d; k <= rows*V)", rows, k, V, kBeamMax);
  hipLaunchKernelGGL(beam_topk_kernel, dim3(1), dim3(kBeamThreads), 0, stream, logits, ld, rows, V,
                     prev, k, out_scores, out_index);
  CAPNET_LAUNCH_CHECK();
  return kOk;
}

// the two expansions with a ban list per row (capnet_beam_topk_banned / capnet_beam_topk_batched_banned): the same body,
// BeamExclList between its log-sum-exp and its selection. bans rows follow the logits rows (the batched form: meta's)
__global__ __launch_bounds__(kBeamThreads) void beam_topk_banned_kernel(float* logits, long ld, int rows, int V,
                                                                        const float* __restrict__ prev, int k,
                                                                        const int* __restrict__ bans, int cap,
                                                                        float* __restrict__ out_scores,
                                                                        long long* __restrict__ out_index) {
  beam_topk_body<BeamExclList>(logits, ld, rows, V, prev, k, out_scores, out_index, BeamExclList{bans, cap});
}

__global__ __launch_bounds__(kBeamThreads) void beam_topk_batched_banned_kernel(
    float* logits, long ld, int V, const float* __restrict__ prev, const int* __restrict__ meta, const int* __restrict__ bans,
    int cap, float* __restrict__ out_scores, long long* __restrict__ out_index) {
  const int row0 = meta[3 * blockIdx.x], rows = meta[3 * blockIdx.x + 1], k = meta[3 * blockIdx.x + 2];
  if (k <= 0 || rows <= 0) return;
  beam_topk_body<BeamExclList>(logits + (long)row0 * ld, ld, rows, V, prev + row0, k, out_scores + (long)blockIdx.x * kBeamMax,
                               out_index + (long)blockIdx.x * kBeamMax, BeamExclList{bans + (long)row0 * (1 + cap), cap});
}

int beam_topk_banned(float* logits, long ld, int rows, int V, const float* prev, int k, const int* bans, int cap,
                     float* out_scores, long long* out_index, hipStream_t stream) {
  CAPNET_REQUIRE(logits && prev && bans && out_scores && out_index, "beam_topk_banned: null argument");
  CAPNET_REQUIRE(rows >= 1 && rows <= kBeamMax && k >= 1 && k <= kBeamMax && V >= 1 && ld >= V && (long)rows * V >= k,
                 "beam_topk_banned: rows=%d k=%d V=%d (rows, k <= %d; k <= rows*V)", rows, k, V, kBeamMax);
  CAPNET_REQUIRE(cap >= 1 && cap <= (1 << 16) && (size_t)bans % 4 == 0, "beam_topk_banned: cap=%d (1 .. 65536), bans 4-byte aligned", cap);
  hipLaunchKernelGGL(beam_topk_banned_kernel, dim3(1), dim3(kBeamThreads), 0, stream, logits, ld, rows, V, prev, k, bans, cap,
                     out_scores, out_index);
  CAPNET_LAUNCH_CHECK();
  return kOk;
}

// ---- beam search with its bookkeeping on the device (capnet.beam.beam_search_device) -------------------------------
// Fixed slots: image i owns rows i k .. i k + k - 1 of the decoder step for the whole search; its live beams are its
// first live[i] slots, in the top-k rank order of the survivors (the order capnet.beam keeps). The state, in 4-byte
// words (L = max_steps + 2 tokens per sequence):
//   [0] live_total  [1..3] unused | live[n] | n_done[n] | scores[n k] f32 | done_score[n k] f32 | done_len[n k] |
//   seq[2][n][k][L] (step s reads buffer (s - 1) & 1 and writes the other) | done_seq[n][k][L]
struct BeamState {
  int *live_total, *live, *n_done, *done_len, *seq, *done_seq;
  float *scores, *done_score;
};
static size_t beam_state_words(int n, int k, int max_steps) {
  const size_t nk = (size_t)n * k;
  return 4 + 2 * (size_t)n + 3 * nk + 3 * nk * (max_steps + 2);
}
__host__ __device__ static inline BeamState beam_state_of(void* beam, int n, int k, int max_steps) {
  const long nk = (long)n * k;
  int* w = static_cast<int*>(beam);
  BeamState s;
  s.live_total = w;
  s.live = w + 4;
  s.n_done = s.live + n;
  s.scores = reinterpret_cast<float*>(s.n_done + n);
  s.done_score = s.scores + nk;
  s.done_len = reinterpret_cast<int*>(s.done_score + nk);
  s.seq = s.done_len + nk;
  s.done_seq = s.seq + 2 * nk * (max_steps + 2);
  return s;
}

// The row trace of a search whose attention maps are wanted (capnet_beam_advance_traced): a buffer of its own BESIDE the
// state, in the sequences' shape -- rows[2][n][k][L] (the buffers swap as seq's do) | done_rows[n][k][L], int32. Entry e
// (1 <= e <= step) of a hypothesis is the slot, within its image, that it occupied when the decoder ran step e: the row
// whose step-e attention preceded its word e. Entry 0 is -1 (the start token has no map).
struct BeamTrace {
  int *rows, *done_rows;   // both null: no trace
};
__host__ __device__ static inline BeamTrace beam_trace_of(void* trace, int n, int k, int max_steps) {
  BeamTrace t;
  t.rows = static_cast<int*>(trace);
  t.done_rows = trace ? t.rows + 2L * n * k * (max_steps + 2) : nullptr;
  return t;
}

__global__ __launch_bounds__(256) void beam_init_kernel(void* beam, int n, int k, int max_steps, int start_token,
                                                        long long* __restrict__ prev_words) {
  const BeamState s = beam_state_of(beam, n, k, max_steps);
  const int L = max_steps + 2, nk = n * k;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < nk; t += gridDim.x * blockDim.x) {
    s.scores[t] = 0.f;
    s.seq[(long)t * L] = start_token;
    prev_words[t] = start_token;
    if (t < n) { s.live[t] = k; s.n_done[t] = 0; }
    if (t == 0) *s.live_total = nk;
  }
}

// what a step does with an image's `picked` best candidates (s_score / s_flat, flat = row in image * V + word, visible to
// the whole workgroup) -- what beam_search_batched does on the host: <end> completes a beam (score and sequence appended to
// the image's completed list, by step then rank), every other beam survives into the next free slot; dead slots still
// take the decoder step, <end> on their own row. `live`: the image's live beams before the step (picked == live unless
// the step had fewer candidates to offer). THREADS: the workgroup's size.
template <int THREADS>
__device__ __forceinline__ void beam_advance_tail(const BeamState& s, int i, int n, int k, int max_steps, int step,
                                                  long long end_token, int V, int live, int picked, const float* s_score,
                                                  const long long* s_flat, long long* __restrict__ next_words,
                                                  long long* __restrict__ parent_rows, const BeamTrace tr = BeamTrace{nullptr, nullptr}) {
  __shared__ int s_parent[kBeamMax], s_word[kBeamMax], s_dst[kBeamMax];   // s_dst: slot, or -1 - index in the completed list
  __shared__ int s_alive;
  const int tid = threadIdx.x, L = max_steps + 2;
  const long row0 = (long)i * k;
  if (live > 0) {
    if (tid == 0) {
      int alive = 0, done = s.n_done[i];
      for (int j = 0; j < picked; ++j) {
        const int w = (int)(s_flat[j] % V);
        s_parent[j] = (int)(s_flat[j] / V);
        s_word[j] = w;
        s_dst[j] = w == end_token ? -1 - done++ : alive++;
      }
      s_alive = alive;
      s.n_done[i] = done;
      s.live[i] = alive;
      if (alive != live) atomicAdd(s.live_total, alive - live);
    }
    __syncthreads();
    // sequences: `step` tokens of the parent, then the word
    const int* seq_in = s.seq + ((long)((step - 1) & 1) * n * k + row0) * L;
    int* seq_out = s.seq + ((long)(step & 1) * n * k + row0) * L;
    int* seq_done = s.done_seq + row0 * L;
    for (int t = tid; t < picked * (step + 1); t += THREADS) {
      const int j = t / (step + 1), e = t % (step + 1);
      int* dst = s_dst[j] >= 0 ? seq_out + (long)s_dst[j] * L : seq_done + (long)(-1 - s_dst[j]) * L;
      dst[e] = e < step ? seq_in[(long)s_parent[j] * L + e] : s_word[j];
    }
    if (tr.rows) {   // the same copy of the parent's row history, then the parent's slot: where this step's map lies
      const int* rows_in = tr.rows + ((long)((step - 1) & 1) * n * k + row0) * L;
      int* rows_out = tr.rows + ((long)(step & 1) * n * k + row0) * L;
      int* rows_done = tr.done_rows + row0 * L;
      for (int t = tid; t < picked * (step + 1); t += THREADS) {
        const int j = t / (step + 1), e = t % (step + 1);
        int* dst = s_dst[j] >= 0 ? rows_out + (long)s_dst[j] * L : rows_done + (long)(-1 - s_dst[j]) * L;
        dst[e] = e == 0 ? -1 : e < step ? rows_in[(long)s_parent[j] * L + e] : s_parent[j];
      }
    }
    if (tid < picked) {
      const int d = s_dst[tid];
      if (d >= 0) {
        s.scores[row0 + d] = s_score[tid];
        next_words[row0 + d] = s_word[tid];
        parent_rows[row0 + d] = row0 + s_parent[tid];
      } else {
        s.done_score[row0 - 1 - d] = s_score[tid];
        s.done_len[row0 - 1 - d] = step + 1;
      }
    }
  }
  // dead slots still take the decoder step: <end> on their own row
  const int alive = live > 0 ? s_alive : 0;
  if (tid >= alive && tid < k) {
    next_words[row0 + tid] = end_token;
    parent_rows[row0 + tid] = row0 + tid;
  }
}

// one step of image blockIdx.x: beam_topk_body over its live rows (row 0 alone at step 1) for its live[i] best, then
// beam_advance_tail
__global__ __launch_bounds__(kBeamThreads) void beam_advance_kernel(
    void* beam, const float* __restrict__ logits, long ld, int V, int n, int k, int max_steps, int step, long long end_token,
    long long* __restrict__ next_words, long long* __restrict__ parent_rows, void* trace) {
  __shared__ float s_score[kBeamMax];
  __shared__ long long s_flat[kBeamMax];
  const BeamState s = beam_state_of(beam, n, k, max_steps);
  const int i = blockIdx.x;
  const long row0 = (long)i * k;
  const int live = s.live[i];
  if (live > 0)
    beam_topk_body<BeamNoExcl>(logits + row0 * ld, ld, step == 1 ? 1 : live, V, s.scores + row0, live, s_score, s_flat);
  beam_advance_tail<kBeamThreads>(s, i, n, k, max_steps, step, end_token, V, live, live, s_score, s_flat, next_words,
                                  parent_rows, beam_trace_of(trace, n, k, max_steps));
}

// beam_advance_kernel under constraints (capnet_beam_advance_constrained): the same body and the same tail, BeamExclState
// on the image's own sequences between the log-sum-exp and the selection. The logits block is written (-INFINITY over the
// excluded words of the rows that compete), so it is neither const nor __restrict__ here.
__global__ __launch_bounds__(kBeamThreads) void beam_advance_constrained_kernel(
    void* beam, float* logits, long ld, int V, int n, int k, int max_steps, int step, long long end_token, int no_repeat_ngram,
    int min_words, const int* __restrict__ banned, int n_banned, long long* __restrict__ next_words,
    long long* __restrict__ parent_rows, void* trace) {
  __shared__ float s_score[kBeamMax];
  __shared__ long long s_flat[kBeamMax];
  const BeamState s = beam_state_of(beam, n, k, max_steps);
  const int i = blockIdx.x, L = max_steps + 2;
  const long row0 = (long)i * k;
  const int live = s.live[i];
  if (live > 0) {
    const BeamExclState excl{s.seq + ((long)((step - 1) & 1) * n * k + row0) * L, L, step, no_repeat_ngram, min_words, end_token,
                             banned, n_banned};
    beam_topk_body<BeamExclState>(logits + row0 * ld, ld, step == 1 ? 1 : live, V, s.scores + row0, live, s_score, s_flat, excl);
  }
  beam_advance_tail<kBeamThreads>(s, i, n, k, max_steps, step, end_token, V, live, live, s_score, s_flat, next_words,
                                  parent_rows, beam_trace_of(trace, n, k, max_steps));
}

// beam_advance_kernel on a step's candidates instead of its logits (capnet_vocab_topk: values / index [n k][k] best first,
// index -1 = nothing; lse [n k]): image blockIdx.x takes its live[i] best of scores[row] - lse[row] + values[row][j] over
// its live rows (row 0 alone at step 1) and j < k, ties to the lower flat index row * V + index -- beam_topk_body's
// selection whenever no two scores tie after rounding, since a row's members of the image's top-live are among that
// row's top-live logits (fp32 addition is monotone). At most 16 x 16 candidates: a thread per candidate, its rank the
// number of candidates that beat it. A padded candidate is never chosen and never an address; an image that is offered
// fewer candidates than it has live beams keeps that many.
constexpr int kBeamTopkThreads = kBeamMax * kBeamMax;
__global__ __launch_bounds__(kBeamTopkThreads) void beam_advance_topk_kernel(
    void* beam, const float* __restrict__ values, const int* __restrict__ index, const float* __restrict__ lse, int V, int n,
    int k, int max_steps, int step, long long end_token, long long* __restrict__ next_words, long long* __restrict__ parent_rows) {
  __shared__ float s_score[kBeamMax];
  __shared__ long long s_flat[kBeamMax];
  __shared__ float s_cv[kBeamTopkThreads];
  __shared__ long long s_cf[kBeamTopkThreads];
  __shared__ int s_valid;
  const BeamState s = beam_state_of(beam, n, k, max_steps);
  const int i = blockIdx.x, tid = threadIdx.x;
  const long row0 = (long)i * k;
  const int live = s.live[i];
  int picked = 0;
  if (live > 0) {
    const int rows = step == 1 ? 1 : live, nc = rows * k;
    if (tid == 0) s_valid = 0;
    __syncthreads();
    float v = -INFINITY;
    long long flat = 0x7fffffffffffffffLL;
    bool ok = false;
    if (tid < nc) {
      const int r = tid / k, j = tid % k;
      const int w = index[(row0 + r) * k + j];
      ok = w >= 0 && w < V;
      if (ok) {
        const float base = s.scores[row0 + r] - lse[row0 + r];
        v = base + values[(row0 + r) * k + j];
        flat = (long long)r * V + w;
        atomicAdd(&s_valid, 1);
      }
    }
    s_cv[tid] = v;
    s_cf[tid] = flat;
    __syncthreads();
    picked = min(live, s_valid);
    if (ok) {
      int rank = 0;
      for (int c = 0; c < nc; ++c) {
        const float ov = s_cv[c];
        const long long of = s_cf[c];
        rank += (of != 0x7fffffffffffffffLL && (ov > v || (ov == v && of < flat))) ? 1 : 0;
      }
      if (rank < picked) { s_score[rank] = v; s_flat[rank] = flat; }
    }
    __syncthreads();
  }
  beam_advance_tail<kBeamTopkThreads>(s, i, n, k, max_steps, step, end_token, V, live, picked, s_score, s_flat, next_words,
                                      parent_rows);
}

// one wave per image: the first maximum of the completed scores in completion order; nothing completed -> [<end>]
__global__ __launch_bounds__(64) void beam_finish_kernel(const void* beam, int n, int k, int max_steps, long long end_token,
                                                         long long* __restrict__ seqs, int* __restrict__ lengths,
                                                         const void* trace, int* __restrict__ rows) {
  const BeamState s = beam_state_of(const_cast<void*>(beam), n, k, max_steps);
  const int i = blockIdx.x, L = max_steps + 2;
  const long row0 = (long)i * k;
  const int done = s.n_done[i];
  int best = 0;
  for (int q = 1; q < done; ++q)
    if (s.done_score[row0 + q] > s.done_score[row0 + best]) best = q;
  const int len = done ? s.done_len[row0 + best] : 1;
  const int* src = s.done_seq + (row0 + best) * L;
  for (int e = threadIdx.x; e < L; e += 64) seqs[(long)i * L + e] = e >= len ? 0 : done ? src[e] : end_token;
  if (threadIdx.x == 0) lengths[i] = len;
  if (rows) {   // the winner's rows as rows of the decoder step, i k + slot; -1 past its last word and for a slot out of range
    const int* rsrc = beam_trace_of(const_cast<void*>(trace), n, k, max_steps).done_rows + (row0 + best) * L;
    for (int e = threadIdx.x; e < max_steps; e += 64) {
      const int slot = done && e + 1 < len ? rsrc[e + 1] : -1;
      rows[(long)i * max_steps + e] = slot >= 0 && slot < k ? (int)row0 + slot : -1;
    }
  }
}

// one wave per image: ALL of its completed hypotheses, best first (capnet_beam_nbest). The key is done_score itself at
// length_penalty 0 -- no division, no powf: rank 0 is then beam_finish's winner bit for bit -- else done_score /
// (done_len - 1)^length_penalty (done_len - 1: the generated words, <end> included). At most 16 hypotheses: a thread per
// hypothesis, its rank the number that beat it (beam_advance_topk_kernel's way), ties to the earlier completion. The
// state is only read. A completed count outside [0, k] is clamped, a recorded slot outside [0, k) gives -1: nothing read
// from the state is an address unchecked.
__global__ __launch_bounds__(64) void beam_nbest_kernel(const void* beam, int n, int k, int max_steps, float length_penalty,
                                                        long long* __restrict__ seqs, int* __restrict__ lengths,
                                                        float* __restrict__ scores, int* __restrict__ counts,
                                                        const void* trace, int* __restrict__ rows) {
  __shared__ float s_key[kBeamMax];
  __shared__ int s_src[kBeamMax];   // rank -> index in the completed list
  const BeamState s = beam_state_of(const_cast<void*>(beam), n, k, max_steps);
  const int i = blockIdx.x, tid = threadIdx.x, L = max_steps + 2;
  const long row0 = (long)i * k;
  const int done = min(max(s.n_done[i], 0), k);
  float key = 0.f;
  if (tid < done) {
    key = s.done_score[row0 + tid];
    if (length_penalty != 0.f) key = key / powf((float)(s.done_len[row0 + tid] - 1), length_penalty);
    s_key[tid] = key;
  }
  if (tid < kBeamMax) s_src[tid] = tid;   // (a NaN key counts nothing: every rank still names a completed hypothesis)
  __syncthreads();
  int rank = 0;
  if (tid < done) {
    for (int q = 0; q < done; ++q) {
      const float ok = s_key[q];
      rank += (ok > key || (ok == key && q < tid)) ? 1 : 0;
    }
  }
  __syncthreads();
  if (tid < done) s_src[rank] = tid;
  __syncthreads();
  for (int t = tid; t < k * L; t += 64) {
    const int r = t / L, e = t % L;
    long long w = 0;
    if (r < done) {
      const long q = row0 + s_src[r];
      if (e < s.done_len[q]) w = s.done_seq[q * L + e];
    }
    seqs[row0 * L + t] = w;
  }
  if (tid < k) {
    const bool has = tid < done;
    const long q = row0 + (has ? s_src[tid] : 0);
    lengths[row0 + tid] = has ? s.done_len[q] : 0;
    scores[row0 + tid] = has ? s.done_score[q] : 0.f;
  }
  if (tid == 0) counts[i] = done;
  if (rows) {   // beam_finish_kernel's rule per hypothesis: i k + slot; -1 past its last word and for a slot out of range
    const int* done_rows = beam_trace_of(const_cast<void*>(trace), n, k, max_steps).done_rows;
    for (int t = tid; t < k * max_steps; t += 64) {
      const int r = t / max_steps, e = t % max_steps;
      int slot = -1;
      if (r < done) {
        const long q = row0 + s_src[r];
        if (e + 1 < s.done_len[q]) slot = done_rows[q * L + e + 1];
      }
      rows[row0 * max_steps + t] = slot >= 0 && slot < k ? (int)row0 + slot : -1;
    }
  }
}

static int beam_check(const char* what, const void* beam, int n, int k, int max_steps) {
  CAPNET_REQUIRE(beam != nullptr, "%s: null beam state", what);
  CAPNET_REQUIRE(n >= 1 && k >= 1 && k <= kBeamMax && max_steps >= 1 && (long)n * k * (max_steps + 2) < (1L << 28),
                 "%s: n=%d k=%d max_steps=%d (n, max_steps >= 1; 1 <= k <= %d)", what, n, k, max_steps, kBeamMax);
  return kOk;
}

size_t beam_state_bytes(int n, int k, int max_steps) {
  if (n < 1 || k < 1 || k > kBeamMax || max_steps < 1) return 0;
  return beam_state_words(n, k, max_steps) * sizeof(int);
}

int beam_init(void* beam, int n, int k, int max_steps, long long start_token, long long* prev_words, hipStream_t stream) {
  if (int rc = beam_check("beam_init", beam, n, k, max_steps)) return rc;
  CAPNET_REQUIRE(prev_words != nullptr, "beam_init: null argument");
  CAPNET_REQUIRE(start_token >= 0 && start_token <= 0x7fffffffLL, "beam_init: start_token %lld", start_token);
  hipLaunchKernelGGL(beam_init_kernel, dim3((n * k + 255) / 256), dim3(256), 0, stream, beam, n, k, max_steps, (int)start_token,
                     prev_words);
  CAPNET_LAUNCH_CHECK();
  return kOk;
}

int beam_constraints_check(const char* who, const BeamConstraints& c) {
  CAPNET_REQUIRE(c.no_repeat_ngram >= 0 && c.no_repeat_ngram <= kNgramMax && c.min_words >= 0 && c.n_banned >= 0 &&
                     c.n_banned <= kBanMax,
                 "%s: no_repeat_ngram=%d (0 .. %d) min_words=%d (>= 0) n_banned=%d (0 .. %d)", who, c.no_repeat_ngram, kNgramMax,
                 c.min_words, c.n_banned, kBanMax);
  CAPNET_REQUIRE((c.banned || !c.n_banned) && (size_t)c.banned % 4 == 0, "%s: banned must be a 4-byte aligned device array", who);
  return kOk;
}

// ---- diverse beam search (Vijayakumar et al. 2016): image i's k beams are D teams of kt = k / D, team g in
// slots g kt .. g kt + kt - 1 -- so the state of a diverse search over n images IS the plain BeamState of n D searches
// of kt beams (state-image i D + g), and init, tail, finish, n-best and the trace are the plain ones. One workgroup per
// image walks its teams in order: team g takes its live best by key = score - strength * c_g(v), c_g(v) the number of
// candidates teams 0 .. g - 1 of the image selected at THIS step whose word is v (<end> counted like any word; a team
// with no live beam selects nothing and adds nothing). The counts are a (word, count) list in LDS, at most k <= 16
// entries, alive until the image's last team; the scores carried forward are unpenalised (BeamPenList).
// every thread reaches every barrier: live is uniform over the workgroup, and a dead team skips the body as a whole.
__device__ __forceinline__ void beam_team_count(const long long* s_flat, int picked, int V, int* s_word, int* s_count,
                                                int* s_words) {
  int m = *s_words;
  for (int j = 0; j < picked; ++j) {
    const int w = (int)(s_flat[j] % V);
    int q = 0;
    while (q < m && s_word[q] != w) ++q;
    if (q < m) ++s_count[q];
    else if (m < kBeamMax) { s_word[m] = w; s_count[m] = 1; ++m; }
  }
  *s_words = m;
}

__global__ __launch_bounds__(kBeamThreads) void beam_advance_diverse_kernel(
    void* beam, void* trace, float* logits, long ld, int V, int n, int k, int D, float strength, int max_steps, int step,
    long long end_token, int no_repeat_ngram, int min_words, const int* __restrict__ banned, int n_banned,
    long long* __restrict__ next_words, long long* __restrict__ parent_rows) {
  __shared__ float s_score[kBeamMax];
  __shared__ long long s_flat[kBeamMax];
  __shared__ int s_pw[kBeamMax], s_pc[kBeamMax], s_pn;
  __shared__ float s_orig[kBeamMax * kBeamMax];
  const int kt = k / D, nq = n * D, L = max_steps + 2;
  const BeamState s = beam_state_of(beam, nq, kt, max_steps);
  const BeamTrace tr = beam_trace_of(trace, nq, kt, max_steps);
  if (threadIdx.x == 0) s_pn = 0;
  __syncthreads();
  for (int g = 0; g < D; ++g) {
    const int q = blockIdx.x * D + g;
    const long row0 = (long)q * kt;
    const int live = s.live[q];
    if (live > 0) {
      const BeamExclState excl{s.seq + ((long)((step - 1) & 1) * nq * kt + row0) * L, L, step, no_repeat_ngram, min_words,
                               end_token, banned, n_banned};
      const BeamPenList pen{s_pw, s_pc, s_pn, strength, s_orig};
      beam_topk_body<BeamExclState, BeamPenList>(logits + row0 * ld, ld, step == 1 ? 1 : live, V, s.scores + row0, live, s_score,
                                                 s_flat, excl, pen);
    }
    beam_advance_tail<kBeamThreads>(s, q, nq, kt, max_steps, step, end_token, V, live, live, s_score, s_flat, next_words,
                                    parent_rows, tr);
    if (live > 0 && threadIdx.x == 0) beam_team_count(s_flat, live, V, s_pw, s_pc, &s_pn);
    __syncthreads();   // the body's and the tail's arrays are the next team's
  }
}

// the host loops' form (capnet_beam_topk_batched_diverse): workgroup i expands image i's D teams in order; meta [n D][3] =
// (first row, rows that compete, live) per (image, team), flat indices local to the team, outputs [n D][16]
__global__ __launch_bounds__(kBeamThreads) void beam_topk_batched_diverse_kernel(
    float* logits, long ld, int V, const float* __restrict__ prev, const int* __restrict__ meta, int D, float strength,
    const int* __restrict__ bans, int cap, float* __restrict__ out_scores, long long* __restrict__ out_index) {
  __shared__ float s_score[kBeamMax];
  __shared__ long long s_flat[kBeamMax];
  __shared__ int s_pw[kBeamMax], s_pc[kBeamMax], s_pn;
  __shared__ float s_orig[kBeamMax * kBeamMax];
  if (threadIdx.x == 0) s_pn = 0;
  __syncthreads();
  for (int g = 0; g < D; ++g) {
    const int q = blockIdx.x * D + g;
    const int row0 = meta[3 * q], rows = meta[3 * q + 1], live = meta[3 * q + 2];
    if (live > 0 && rows > 0 && live <= kBeamMax && rows <= kBeamMax) {   // (meta lives on the device: bounded here)
      const BeamExclListOrNone excl{bans ? bans + (long)row0 * (1 + cap) : nullptr, cap};
      const BeamPenList pen{s_pw, s_pc, s_pn, strength, s_orig};
      beam_topk_body<BeamExclListOrNone, BeamPenList>(logits + (long)row0 * ld, ld, rows, V, prev + row0, live, s_score, s_flat,
                                                      excl, pen);
      if (threadIdx.x < live) {
        out_scores[(long)q * kBeamMax + threadIdx.x] = s_score[threadIdx.x];
        out_index[(long)q * kBeamMax + threadIdx.x] = s_flat[threadIdx.x];
      }
      if (threadIdx.x == 0) beam_team_count(s_flat, live, V, s_pw, s_pc, &s_pn);
    }
    __syncthreads();
  }
}

// ---- forced words (Post & Vilar 2018, dynamic beam allocation): every completed hypothesis contains all F <= 4
// forced ids. A row's met mask (bit f: forced[f] occurs among its words, <start> apart) is recomputed each step -- the
// device form scans the row's `step` tokens in BeamState.seq, a thread per (row, forced id); the host form is handed it.
// BeamExclForced is the exclusion: the inner functor's, then <end> on every row whose mask is not full. BeamForcedPool
// runs behind the `live` plain passes, on their result in LDS:
//   pool  [0, 16)   the plain selection (part 1)
//         [16, 80)  (row r, forced[f]) at 16 + 4 r + f where bit f of r's mask is clear and the logit is not -inf (part 2)
//         [80, 96)  row r's best word that is not -inf at 80 + r: one more pass over the block, each row split over the
//                   waves (part 3)
//   bank  the popcount of (the row's mask | the bits of the forced ids the word equals)
//   an entry whose flat index an earlier entry holds leaves; within a bank the rank of an entry is the number of entries
//   that beat it (score descending, ties to the lower flat index: a total order, flat indices being distinct by now);
//   one thread then visits the banks F, F - 1 .. 0, F .. and takes each one's best untaken entry until `live` are taken
//   or the pool is empty. The order of taking is the output order.
// Scores are (prev - lse) + logit, the plain selection's expression on the same operands: the same bits. Static LDS: the
// pool's 96 x (4 + 8 + 4 + 4) bytes, the 5 x 96 rank table, part 3's 16 x 16 partial bests (3 KB) and a few counters, 6.9 KB
// beside the body's own.
constexpr int kForcedMax = 4, kForcedPool = kBeamMax + kBeamMax * kForcedMax + kBeamMax;

template <class Inner>
struct BeamExclForced {
  typedef float* logits_t;
  static constexpr bool kActive = true;
  Inner inner;
  const int* tok;        // the image's rows of BeamState.seq ([k][L], `step` tokens each), or null: met_in holds the masks
  int L, step;
  const int* met_in;     // int32 per competing row (the host form), or null
  const int* forced;     // DEVICE array [n_forced]
  int n_forced;
  long long end_token;
  int* s_met;            // LDS [kBeamMax]: the masks, for the pool behind the selection too
  __device__ __forceinline__ void operator()(float* logits, long ld, int rows, int V) const {
    const int tid = threadIdx.x, full = (1 << n_forced) - 1;
    if (tid < kBeamMax) s_met[tid] = (met_in && tid < rows) ? (met_in[tid] & full) : 0;
    __syncthreads();
    if (tok) {
      for (int t = tid; t < rows * n_forced; t += kBeamThreads) {
        const int r = t / n_forced, f = t % n_forced, w = forced[f];
        const int* q = tok + (long)r * L;
        bool hit = false;
        for (int e = 1; e < step; ++e) hit |= q[e] == w;
        if (hit) atomicOr(&s_met[r], 1 << f);
      }
      __syncthreads();
    }
    inner(logits, ld, rows, V);
    if (tid < rows && s_met[tid] != full && end_token >= 0 && end_token < V) logits[(long)tid * ld + end_token] = -INFINITY;
  }
};

struct BeamForcedPool {
  static constexpr bool kActive = true;
  const int* forced;     // DEVICE array [n_forced]
  int n_forced;
  const int* s_met;      // LDS [kBeamMax], BeamExclForced's
  int* s_picked;         // LDS: how many were taken (live, unless the pool held fewer)
  __device__ __forceinline__ void operator()(const float* logits, long ld, int rows, int V, const float* __restrict__ prev,
                                             const float* s_lse, int live, float* sel_score, long long* sel_flat) const {
    __shared__ float p_score[kForcedPool];
    __shared__ long long p_flat[kForcedPool];
    __shared__ int p_valid[kForcedPool], p_bank[kForcedPool];
    __shared__ int s_at[(kForcedMax + 1) * kForcedPool], s_cnt[kForcedMax + 1], s_next[kForcedMax + 1];
    constexpr int kWaves = kBeamThreads / 64;
    __shared__ float s_pv[kBeamMax * kWaves];      // part 3: the waves' partial bests per row
    __shared__ long s_pi[kBeamMax * kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long total = (long)rows * V;
    // parts 1 and 2: a thread per slot
    if (tid < kBeamMax + kBeamMax * kForcedMax) {
      float v = 0.f;
      long long flat = 0;
      bool ok = false;
      if (tid < kBeamMax) {
        if (tid < live) {
          v = sel_score[tid];
          flat = sel_flat[tid];
          ok = flat >= 0 && flat < total && v > -INFINITY;
        }
      } else {
        const int r = (tid - kBeamMax) / kForcedMax, f = (tid - kBeamMax) % kForcedMax;
        if (r < rows && f < n_forced && !((s_met[r] >> f) & 1)) {
          const int w = forced[f];
          if (w >= 0 && w < V) {
            const float x = logits[(long)r * ld + w];
            v = (prev[r] - s_lse[r]) + x;
            flat = (long long)r * V + w;
            ok = x > -INFINITY && v > -INFINITY;
          }
        }
      }
      p_score[tid] = v;
      p_flat[tid] = flat;
      p_valid[tid] = ok ? 1 : 0;
    }
    if (tid <= kForcedMax) { s_cnt[tid] = 0; s_next[tid] = 0; }
    // part 3: every row's best word in one pass over the block -- each row split over the workgroup's waves (a wave's 64
    // lanes alone on a row of 8192 would make 128 dependent trips), the waves' partial bests in LDS, one barrier for all
    // rows, then thread r folds row r's partials
    for (int r = 0; r < rows; ++r) {
      const float* p = logits + (long)r * ld;
      const float base = prev[r] - s_lse[r];
      float bv = -INFINITY;
      long bi = 0x7fffffffffffffffL;
      for (int v = tid; v < V; v += kBeamThreads) {
        const float x = p[v];
        if (x > -INFINITY) beam_better(base + x, (long)r * V + v, bv, bi);
      }
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o);
        const long oi = __shfl_xor(bi, o);
        beam_better(ov, oi, bv, bi);
      }
      if (lane == 0) { s_pv[r * kWaves + wave] = bv; s_pi[r * kWaves + wave] = bi; }
    }
    __syncthreads();
    if (tid < kBeamMax) {
      float bv = -INFINITY;
      long bi = 0x7fffffffffffffffL;
      if (tid < rows)
        for (int w = 0; w < kWaves; ++w) beam_better(s_pv[tid * kWaves + w], s_pi[tid * kWaves + w], bv, bi);
      const bool ok = tid < rows && bi < total && bv > -INFINITY;
      p_score[kForcedPool - kBeamMax + tid] = bv;
      p_flat[kForcedPool - kBeamMax + tid] = ok ? bi : 0;
      p_valid[kForcedPool - kBeamMax + tid] = ok ? 1 : 0;
    }
    __syncthreads();
    // the bank of every entry; an entry whose flat index an earlier entry holds leaves
    if (tid < kForcedPool) {
      int bank = -1;
      if (p_valid[tid]) {
        const long long flat = p_flat[tid];
        bool dup = false;
        for (int e = 0; e < tid; ++e) dup |= p_valid[e] && p_flat[e] == flat;
        if (!dup) {
          const int r = (int)(flat / V), w = (int)(flat % V);
          int m = s_met[r];
          for (int f = 0; f < n_forced; ++f)
            if (forced[f] == w) m |= 1 << f;
          bank = __popc(m);
        }
      }
      p_bank[tid] = bank;
    }
    __syncthreads();
    // the rank within the bank, by counting
    if (tid < kForcedPool && p_bank[tid] >= 0) {
      const int bank = p_bank[tid];
      const float v = p_score[tid];
      const long long flat = p_flat[tid];
      int rank = 0;
      for (int e = 0; e < kForcedPool; ++e) {
        const float ov = p_score[e];
        rank += (p_bank[e] == bank && (ov > v || (ov == v && p_flat[e] < flat))) ? 1 : 0;
      }
      s_at[bank * kForcedPool + rank] = tid;
      atomicAdd(&s_cnt[bank], 1);
    }
    __syncthreads();
    // the walk: banks F, F - 1 .. 0, F ..; the order of taking is the output order
    if (tid == 0) {
      int have = 0;
      for (int b = 0; b <= n_forced; ++b) have += s_cnt[b];
      const int target = min(live, have);
      int taken = 0, b = n_forced;
      while (taken < target) {
        const int q = s_next[b];
        if (q < s_cnt[b]) {
          const int e = s_at[b * kForcedPool + q];
          s_next[b] = q + 1;
          sel_score[taken] = p_score[e];
          sel_flat[taken] = p_flat[e];
          ++taken;
        }
        b = b == 0 ? n_forced : b - 1;
      }
      *s_picked = taken;
    }
    __syncthreads();
  }
};

// one step of image blockIdx.x under forced words (capnet_beam_advance_forced): beam_advance_constrained_kernel with the
// met masks, the <end> exclusion and the pool around its selection; the tail is used as it is
__global__ __launch_bounds__(kBeamThreads) void beam_advance_forced_kernel(
    void* beam, void* trace, float* logits, long ld, int V, int n, int k, int max_steps, int step, long long end_token,
    int no_repeat_ngram, int min_words, const int* __restrict__ banned, int n_banned, const int* __restrict__ forced,
    int n_forced, long long* __restrict__ next_words, long long* __restrict__ parent_rows) {
  __shared__ float s_score[kBeamMax];
  __shared__ long long s_flat[kBeamMax];
  __shared__ int s_met[kBeamMax], s_picked;
  const BeamState s = beam_state_of(beam, n, k, max_steps);
  const int i = blockIdx.x, L = max_steps + 2;
  const long row0 = (long)i * k;
  const int live = s.live[i];
  int picked = 0;
  if (live > 0) {
    const int* tok = s.seq + ((long)((step - 1) & 1) * n * k + row0) * L;
    const BeamExclForced<BeamExclState> excl{
        BeamExclState{tok, L, step, no_repeat_ngram, min_words, end_token, banned, n_banned}, tok, L, step, nullptr, forced,
        n_forced, end_token, s_met};
    beam_topk_body<BeamExclForced<BeamExclState>, BeamNoPen, BeamForcedPool>(
        logits + row0 * ld, ld, step == 1 ? 1 : live, V, s.scores + row0, live, s_score, s_flat, excl, BeamNoPen(),
        BeamForcedPool{forced, n_forced, s_met, &s_picked});
    picked = s_picked;
  }
  beam_advance_tail<kBeamThreads>(s, i, n, k, max_steps, step, end_token, V, live, picked, s_score, s_flat, next_words,
                                  parent_rows, beam_trace_of(trace, n, k, max_steps));
}

// the host loops' form (capnet_beam_topk_batched_forced): meta as capnet_beam_topk_batched's; bans nullable; met int32 per
// logits row; outputs [n][16], the first `live` entries of a row set (fewer where the pool held fewer: the rest is
// -inf / -1)
__global__ __launch_bounds__(kBeamThreads) void beam_topk_batched_forced_kernel(
    float* logits, long ld, int V, const float* __restrict__ prev, const int* __restrict__ meta, const int* __restrict__ bans,
    int cap, const int* __restrict__ met, const int* __restrict__ forced, int n_forced, long long end_token,
    float* __restrict__ out_scores, long long* __restrict__ out_index) {
  __shared__ float s_score[kBeamMax];
  __shared__ long long s_flat[kBeamMax];
  __shared__ int s_met[kBeamMax], s_picked;
  const int row0 = meta[3 * blockIdx.x], rows = meta[3 * blockIdx.x + 1], live = meta[3 * blockIdx.x + 2];
  if (live <= 0 || rows <= 0 || live > kBeamMax || rows > kBeamMax) return;   // (meta lives on the device: bounded here)
  const BeamExclForced<BeamExclListOrNone> excl{
      BeamExclListOrNone{bans ? bans + (long)row0 * (1 + cap) : nullptr, cap}, nullptr, 0, 0, met + row0, forced, n_forced,
      end_token, s_met};
  beam_topk_body<BeamExclForced<BeamExclListOrNone>, BeamNoPen, BeamForcedPool>(
      logits + (long)row0 * ld, ld, rows, V, prev + row0, live, s_score, s_flat, excl, BeamNoPen(),
      BeamForcedPool{forced, n_forced, s_met, &s_picked});
  if (threadIdx.x < live) {
    const bool has = threadIdx.x < s_picked;
    out_scores[(long)blockIdx.x * kBeamMax + threadIdx.x] = has ? s_score[threadIdx.x] : -INFINITY;
    out_index[(long)blockIdx.x * kBeamMax + threadIdx.x] = has ? s_flat[threadIdx.x] : -1;
  }
}

int beam_forced_check(const char* who, const BeamConstraints& c) {
  CAPNET_REQUIRE(c.n_forced >= 1 && c.n_forced <= kForcedMax && c.forced && (size_t)c.forced % 4 == 0,
                 "%s: n_forced=%d (1 .. %d), forced a 4-byte aligned device array", who, c.n_forced, kForcedMax);
  return kOk;
}

// ---- per-image rules: the rule of a step as a row of a device table instead of kernel arguments. rules int32
// [n][kBeamRuleWords]: word 0 no_repeat_ngram | 1 min_words | 2 n_banned | 3 n_forced | 4 .. 35 banned | 36 .. 39 forced;
// a row of zeros is no rule. The host cannot read the table, so every count is clamped to its range as it is read: whatever
// the table holds, banned and forced are indexed inside the row. The row's address depends on blockIdx alone, so what is
// read from it is uniform over the workgroup and so is every branch taken on it.
constexpr int kRuleBanned = 4, kRuleForced = kRuleBanned + kBanMax;
static_assert(kRuleForced + kForcedMax == kBeamRuleWords, "the rule row: 4 counts, the banned words, the forced ids");

struct BeamRule {
  int g, min_words, n_banned, n_forced;
  const int *banned, *forced;   // into the row
  __device__ __forceinline__ bool excludes() const { return (g | min_words | n_banned) != 0; }
};

__device__ __forceinline__ BeamRule beam_rule_of(const int* __restrict__ rules, int image) {
  const int* row = rules + (long)image * kBeamRuleWords;
  BeamRule r;
  r.g = min(max(row[0], 0), kNgramMax);
  r.min_words = max(row[1], 0);
  r.n_banned = min(max(row[2], 0), kBanMax);
  r.n_forced = min(max(row[3], 0), kForcedMax);
  r.banned = row + kRuleBanned;
  r.forced = row + kRuleForced;
  return r;
}

// one step of image blockIdx.x under ITS OWN rule (capnet_beam_advance_rules): the row decides, for the whole workgroup,
// between the three selections of the kernels above -- forced ids: beam_advance_forced_kernel's; else anything excluded:
// beam_advance_constrained_kernel's; else beam_advance_kernel's -- each the same beam_topk_body instance on the same
// functors, built from the row where those kernels build them from their arguments. The tail is used as it is.
__global__ __launch_bounds__(kBeamThreads) void beam_advance_rules_kernel(
    void* beam, void* trace, float* logits, long ld, int V, int n, int k, int max_steps, int step, long long end_token,
    const int* __restrict__ rules, long long* __restrict__ next_words, long long* __restrict__ parent_rows) {
  __shared__ float s_score[kBeamMax];
  __shared__ long long s_flat[kBeamMax];
  __shared__ int s_met[kBeamMax], s_picked;
  const BeamState s = beam_state_of(beam, n, k, max_steps);
  const int i = blockIdx.x, L = max_steps + 2;
  const long row0 = (long)i * k;
  const BeamRule r = beam_rule_of(rules, i);   // (in front of the branch on live: the two loads are in flight together)
  const int live = s.live[i];
  int picked = live;
  if (live > 0) {
    const int* tok = s.seq + ((long)((step - 1) & 1) * n * k + row0) * L;
    const int rows = step == 1 ? 1 : live;
    const BeamExclState own{tok, L, step, r.g, r.min_words, end_token, r.banned, r.n_banned};
    if (r.n_forced > 0) {
      const BeamExclForced<BeamExclState> excl{own, tok, L, step, nullptr, r.forced, r.n_forced, end_token, s_met};
      beam_topk_body<BeamExclForced<BeamExclState>, BeamNoPen, BeamForcedPool>(
          logits + row0 * ld, ld, rows, V, s.scores + row0, live, s_score, s_flat, excl, BeamNoPen(),
          BeamForcedPool{r.forced, r.n_forced, s_met, &s_picked});
      picked = s_picked;
    } else if (r.excludes()) {
      beam_topk_body<BeamExclState>(logits + row0 * ld, ld, rows, V, s.scores + row0, live, s_score, s_flat, own);
    } else {
      beam_topk_body<BeamNoExcl>(logits + row0 * ld, ld, rows, V, s.scores + row0, live, s_score, s_flat);
    }
  }
  beam_advance_tail<kBeamThreads>(s, i, n, k, max_steps, step, end_token, V, live, picked, s_score, s_flat, next_words,
                                  parent_rows, beam_trace_of(trace, n, k, max_steps));
}

// the host loops' form (capnet_beam_topk_batched_rules): beam_topk_batched_forced_kernel with the forced ids and their count
// read from image blockIdx.x's row; bans (nullable) and met per logits row are Python's, built from each row's own image's
// rule. An image without forced ids takes the banned selection on its rows, the plain one where bans is null. Outputs as
// the forced form's: `live` entries of a row set, -inf / -1 where the pool held fewer.
__global__ __launch_bounds__(kBeamThreads) void beam_topk_batched_rules_kernel(
    float* logits, long ld, int V, const float* __restrict__ prev, const int* __restrict__ meta, const int* __restrict__ bans,
    int cap, const int* __restrict__ met, const int* __restrict__ rules, long long end_token, float* __restrict__ out_scores,
    long long* __restrict__ out_index) {
  __shared__ float s_score[kBeamMax];
  __shared__ long long s_flat[kBeamMax];
  __shared__ int s_met[kBeamMax], s_picked;
  const int row0 = meta[3 * blockIdx.x], rows = meta[3 * blockIdx.x + 1], live = meta[3 * blockIdx.x + 2];
  if (live <= 0 || rows <= 0 || live > kBeamMax || rows > kBeamMax) return;   // (meta lives on the device: bounded here)
  const BeamRule r = beam_rule_of(rules, blockIdx.x);
  const BeamExclListOrNone own{bans ? bans + (long)row0 * (1 + cap) : nullptr, cap};
  int picked = live;
  if (r.n_forced > 0) {
    const BeamExclForced<BeamExclListOrNone> excl{own, nullptr, 0, 0, met + row0, r.forced, r.n_forced, end_token, s_met};
    beam_topk_body<BeamExclForced<BeamExclListOrNone>, BeamNoPen, BeamForcedPool>(
        logits + (long)row0 * ld, ld, rows, V, prev + row0, live, s_score, s_flat, excl, BeamNoPen(),
        BeamForcedPool{r.forced, r.n_forced, s_met, &s_picked});
    picked = s_picked;
  } else {
    beam_topk_body<BeamExclListOrNone>(logits + (long)row0 * ld, ld, rows, V, prev + row0, live, s_score, s_flat, own);
  }
  if (threadIdx.x < live) {
    const bool has = threadIdx.x < picked;
    out_scores[(long)blockIdx.x * kBeamMax + threadIdx.x] = has ? s_score[threadIdx.x] : -INFINITY;
    out_index[(long)blockIdx.x * kBeamMax + threadIdx.x] = has ? s_flat[threadIdx.x] : -1;
  }
}

int beam_rules_check(const char* who, const int* rules) {
  CAPNET_REQUIRE(rules != nullptr && (size_t)rules % 16 == 0,
                 "%s: rules must be a 16-byte aligned device table of int32 [n][%d]", who, kBeamRuleWords);
  return kOk;
}

// ---- the two launchers of the selection step. Both choose the kernel by WHICH options are given, never by what they
// hold: a rule table without teams -> the per-image kernel; teams -> the diverse kernel; else forced ids (n_forced != 0) -> the forced kernel; else constraints (a ban list)
// -> the constrained (banned) kernel; else the plain kernel, which only reads the logits. `who` is the caller's name, in
// front of every message.
static int beam_team_range_check(const char* who, int D, float strength) {
  CAPNET_REQUIRE(D >= 1 && D <= kBeamMax, "%s: teams=%d (1 .. %d)", who, D, kBeamMax);
  CAPNET_REQUIRE(strength >= 0.f && strength <= 3.0e38f, "%s: strength must be finite and >= 0", who);
  return kOk;
}

int beam_teams_check(const char* who, int k, int D, float strength) {
  if (int rc = beam_team_range_check(who, D, strength)) return rc;
  CAPNET_REQUIRE(k >= D && k <= kBeamMax && k % D == 0, "%s: teams=%d must divide k=%d (k <= %d)", who, D, k, kBeamMax);
  return kOk;
}

// one step on the device state; with teams, `beam` and `trace` are those of n D searches of k / D beams
int beam_advance(const char* who, void* beam, float* logits, long ld, int V, int n, int k, int max_steps, int step,
                 long long end_token, const BeamConstraints* con, const BeamTeams* teams, long long* next_words,
                 long long* parent_rows, void* trace, hipStream_t stream) {
  const bool per_image = con && con->rules && !teams;   // (the table replaces the scalar fields, which are then not read)
  const bool forced = con && con->n_forced && !teams && !per_image;
  int D = 1;
  if (teams) {
    if (int rc = beam_teams_check(who, k, teams->teams, teams->strength)) return rc;
    CAPNET_REQUIRE(n >= 1 && n <= (1 << 24), "%s: n=%d teams=%d", who, n, teams->teams);
    D = teams->teams;
  }
  if (per_image)
    if (int rc = beam_rules_check(who, con->rules)) return rc;
  if (int rc = beam_check(who, beam, n * D, k / D, max_steps)) return rc;
  if (con && !per_image)
    if (int rc = beam_constraints_check(who, *con)) return rc;
  if (forced)
    if (int rc = beam_forced_check(who, *con)) return rc;
  CAPNET_REQUIRE(logits && next_words && parent_rows && (size_t)trace % 4 == 0, "%s: null argument or trace alignment", who);
  CAPNET_REQUIRE(V >= 1 && k <= V && ld >= V && step >= 1 && step <= max_steps,
                 "%s: V=%d k=%d ld=%ld step=%d max_steps=%d (k <= V <= ld; 1 <= step <= max_steps)", who, V, k, ld, step, max_steps);
  const BeamConstraints c = con ? *con : BeamConstraints{0, 0, nullptr, 0};
  const dim3 grid(n), block(kBeamThreads);
  if (per_image)
    hipLaunchKernelGGL(beam_advance_rules_kernel, grid, block, 0, stream, beam, trace, logits, ld, V, n, k, max_steps, step,
                       end_token, c.rules, next_words, parent_rows);
  else if (teams)
    hipLaunchKernelGGL(beam_advance_diverse_kernel, grid, block, 0, stream, beam, trace, logits, ld, V, n, k, D, teams->strength,
                       max_steps, step, end_token, c.no_repeat_ngram, c.min_words, c.banned, c.n_banned, next_words, parent_rows);
  else if (forced)
    hipLaunchKernelGGL(beam_advance_forced_kernel, grid, block, 0, stream, beam, trace, logits, ld, V, n, k, max_steps, step,
                       end_token, c.no_repeat_ngram, c.min_words, c.banned, c.n_banned, c.forced, c.n_forced, next_words,
                       parent_rows);
  else if (con)
    hipLaunchKernelGGL(beam_advance_constrained_kernel, grid, block, 0, stream, beam, logits, ld, V, n, k, max_steps, step,
                       end_token, c.no_repeat_ngram, c.min_words, c.banned, c.n_banned, next_words, parent_rows, trace);
  else
    hipLaunchKernelGGL(beam_advance_kernel, grid, block, 0, stream, beam, logits, ld, V, n, k, max_steps, step, end_token,
                       next_words, parent_rows, trace);
  CAPNET_LAUNCH_CHECK();
  return kOk;
}

// the host loops' form. meta: DEVICE array [n][3] = (first row, rows that compete, k) per image -- per (image, team), [n D][3],
// with teams -- rows and k <= 16 (the caller checks: the values live on the device); outputs [n][16] ([n D][16]). bans
// (with cap) nullable; met: int32 per logits row, required with forced ids and with rules (the per-image table, which then
// gives every image its forced ids; forced / n_forced are not read).
int beam_topk_batched(const char* who, float* logits, long ld, int V, const float* prev, const int* meta, int n, const int* bans,
                      int cap, const BeamTeams* teams, const int* met, const int* forced, int n_forced, long long end_token,
                      float* out_scores, long long* out_index, hipStream_t stream, const int* rules) {
  const bool per_image = rules && !teams;
  const bool forced_form = n_forced && !teams && !per_image;
  CAPNET_REQUIRE(logits && prev && meta && out_scores && out_index && n >= 0 && V >= 1 && ld >= V &&
                     (met || !(forced_form || per_image)),
                 "%s: bad argument", who);
  if (teams)
    if (int rc = beam_team_range_check(who, teams->teams, teams->strength)) return rc;
  CAPNET_REQUIRE(!bans || (cap >= 1 && cap <= (1 << 16) && (size_t)bans % 4 == 0), "%s: cap=%d (1 .. 65536), bans 4-byte aligned", who,
                 cap);
  if (forced_form) {
    CAPNET_REQUIRE((size_t)met % 4 == 0, "%s: met must be 4-byte aligned", who);
    if (int rc = beam_forced_check(who, BeamConstraints{0, 0, nullptr, 0, forced, n_forced})) return rc;
  }
  if (per_image) {
    CAPNET_REQUIRE((size_t)met % 4 == 0, "%s: met must be 4-byte aligned", who);
    if (int rc = beam_rules_check(who, rules)) return rc;
  }
  if (n == 0) return kOk;
  const dim3 grid(n), block(kBeamThreads);
  if (per_image)
    hipLaunchKernelGGL(beam_topk_batched_rules_kernel, grid, block, 0, stream, logits, ld, V, prev, meta, bans, cap, met, rules,
                       end_token, out_scores, out_index);
  else if (teams)
    hipLaunchKernelGGL(beam_topk_batched_diverse_kernel, grid, block, 0, stream, logits, ld, V, prev, meta, teams->teams,
                       teams->strength, bans, cap, out_scores, out_index);
  else if (forced_form)
    hipLaunchKernelGGL(beam_topk_batched_forced_kernel, grid, block, 0, stream, logits, ld, V, prev, meta, bans, cap, met, forced,
                       n_forced, end_token, out_scores, out_index);
  else if (bans)
    hipLaunchKernelGGL(beam_topk_batched_banned_kernel, grid, block, 0, stream, logits, ld, V, prev, meta, bans, cap, out_scores,
                       out_index);
  else
    hipLaunchKernelGGL(beam_topk_batched_kernel, grid, block, 0, stream, logits, ld, V, prev, meta, out_scores, out_index);
  CAPNET_LAUNCH_CHECK();
  return kOk;
}

size_t beam_trace_bytes(int n, int k, int max_steps) {
  if (n < 1 || k < 1 || k > kBeamMax || max_steps < 1) return 0;
  return 3 * (size_t)n * k * (max_steps + 2) * sizeof(int);
}

int beam_advance_topk(void* beam, const float* values, const int* index, const float* lse, int V, int n, int k, int max_steps,
                      int step, long long end_token, long long* next_words, long long* parent_rows, hipStream_t stream) {
  if (int rc = beam_check("beam_advance_topk", beam, n, k, max_steps)) return rc;
  CAPNET_REQUIRE(values && index && lse && next_words && parent_rows, "beam_advance_topk: null argument");
  CAPNET_REQUIRE(V >= 1 && k <= V && step >= 1 && step <= max_steps,
                 "beam_advance_topk: V=%d k=%d step=%d max_steps=%d (k <= V; 1 <= step <= max_steps)", V, k, step, max_steps);
  hipLaunchKernelGGL(beam_advance_topk_kernel, dim3(n), dim3(kBeamTopkThreads), 0, stream, beam, values, index, lse, V, n, k,
                     max_steps, step, end_token, next_words, parent_rows);
  CAPNET_LAUNCH_CHECK();
  return kOk;
}

int beam_finish(const void* beam, int n, int k, int max_steps, long long end_token, long long* seqs, int* lengths,
                hipStream_t stream, const void* trace, int* rows) {
  if (int rc = beam_check("beam_finish", beam, n, k, max_steps)) return rc;
  CAPNET_REQUIRE(seqs && lengths, "beam_finish: null argument");
  CAPNET_REQUIRE(!trace == !rows, "beam_finish: the trace and the rows go together");
  hipLaunchKernelGGL(beam_finish_kernel, dim3(n), dim3(64), 0, stream, beam, n, k, max_steps, end_token, seqs, lengths, trace,
                     rows);
  CAPNET_LAUNCH_CHECK();
  return kOk;
}

int beam_nbest(const void* beam, int n, int k, int max_steps, float length_penalty, long long* seqs, int* lengths,
               float* scores, int* counts, hipStream_t stream, const void* trace, int* rows) {
  if (int rc = beam_check("beam_nbest", beam, n, k, max_steps)) return rc;
  CAPNET_REQUIRE(seqs && lengths && scores && counts, "beam_nbest: null argument");
  CAPNET_REQUIRE((size_t)beam % 4 == 0 && (size_t)seqs % 8 == 0 && (size_t)lengths % 4 == 0 && (size_t)scores % 4 == 0 &&
                     (size_t)counts % 4 == 0,
                 "beam_nbest: the state, lengths, scores and counts must be 4-byte aligned, seqs 8-byte aligned");
  CAPNET_REQUIRE(std::isfinite(length_penalty), "beam_nbest: length_penalty must be finite");
  CAPNET_REQUIRE(!trace == !rows, "beam_nbest: the trace and the rows go together");
  hipLaunchKernelGGL(beam_nbest_kernel, dim3(n), dim3(64), 0, stream, beam, n, k, max_steps, length_penalty, seqs, lengths,
                     scores, counts, trace, rows);
  CAPNET_LAUNCH_CHECK();
  return kOk;
}

int beam_live(const void* beam, int n, int k, int max_steps, const int** live_total, const int** live, const float** scores) {
  if (int rc = beam_check("beam_live", beam, n, k, max_steps)) return rc;
  const BeamState s = beam_state_of(const_cast<void*>(beam), n, k, max_steps);
  if (live_total) *live_total = s.live_total;
  if (live) *live = s.live;
  if (scores) *scores = s.scores;
  return kOk;
}

// the hypotheses step `step` (1-based) reads: seq[(step - 1) & 1], [n k] rows of max_steps + 2 int32, `step` tokens each with
// <start> first -- what BeamExclState reads, for sample_exclude.hip's mask kernel
int beam_tokens(const void* beam, int n, int k, int max_steps, int step, const int** tokens) {
  if (int rc = beam_check("beam_tokens", beam, n, k, max_steps)) return rc;
  CAPNET_REQUIRE(step >= 1 && step <= max_steps && tokens, "beam_tokens: step=%d of %d", step, max_steps);
  const BeamState s = beam_state_of(const_cast<void*>(beam), n, k, max_steps);
  *tokens = s.seq + (long)((step - 1) & 1) * n * k * (max_steps + 2);
  return kOk;
}

}  // namespace capnet
