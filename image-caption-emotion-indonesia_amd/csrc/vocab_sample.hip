// Sampled decoding: a draw from softmax(logit / T) per row in ONE launch, the logits never in memory (capnet_vocab_sample,
// capnet_sample_pick, capnet_sample_rows; the sampling loops around them: decode_loops.hip).
//   z[r][v] = h[r] . W[v] + b[v]        h [rows][H], W [V][H] (nn.Linear), b [V]
//   s = z inv_T,  key = s + sample_gumbel(sample_uniform(seed, step, row0 + r, v))          (sample_rng.h)
//   (greedy_stride > 0: every greedy_stride-th row is a greedy row, key = s, and the drawn rows keep the noise rows they have
//   without it: vs_row_key in sample_key.h, which every kernel here takes its keys from)
//   tok[r] = argmax_v key (ties to the lower v),  logp[r] = s[tok] - log sum_v exp(s)
// Gumbel-max: the argmax of the noised scaled logits IS a draw from softmax(z / T), so sampling is vocab_argmax with
// counter-based noise in the epilogue; no prefix sum over the vocabulary. The noise is a pure function of (seed, step, row,
// v): the token does not depend on which workgroup arrives last, nor on how a caller splits its rows over launches (row0).
//
// The mapping and the hand-off are vocab_core.h's (one group). Per row the workgroup emits
//   its best (key, index) under the total order (one packed 8-byte word) and that entry's s, and
//   vocab_topk's m_w = the maximum of its pickable s, s_w = sum expf(s - m_w) over them (one packed 8-byte word).
// A logit that is NaN or -inf, or lies beyond V, is not pickable: never drawn, and it adds nothing to s_w. With an exclusion
// mask (sample_exclude.hip) an entry whose bit is set is not pickable either: the draw and logp are those of the distribution
// renormalised over the allowed entries.
// The last arriver merges a wave per row, the workgroups across its lanes: the winner under the total order; M = max m_w,
// S = sum s_w expf(m_w - M) with lane l adding workgroups l, l + 64, ... in that order and the lanes then combined by the
// xor tree, lse = M + logf(S): the same bits whoever arrives last (a rounded product and a sum here, a fused multiply-add
// in vocab_topk.hip: each kernel keeps its own merge and its own rounding). A row with nothing to pick yields token 0 and
// logp = -inf.
//
// sample_pick_kernel: the same draw among the k candidates of vocab_topk's (values, index) -- top-k sampling. The noise is
// keyed by the candidate's VOCABULARY index, so k = V would draw what the full kernel draws; logp is renormalised over the
// k candidates; padding slots (-inf, -1) are never picked.
// sample_rows_kernel: the same draw from a [rows][ld] logits block in memory, one workgroup per row (the composed route).
#include "common.h"
#include "kernels.h"
#include "vocab_core.h"
#include "sample_key.h"   // vs_scaled, vs_key; no FMA contraction in this file

namespace capnet {

struct VocabSampleArgs {
  const float* h;            // [rows][H]
  const float* w;            // [V][H]
  const float* b;            // [V] or null
  unsigned long long* best;  // [workgroups][rows]: (key bits << 32) | index
  unsigned long long* stat;  // [workgroups][rows]: (m_w bits << 32) | s_w bits
  unsigned* sval;            // [workgroups][rows]: the best entry's scaled logit
  int* counter;              // zero before the first use, zero again when the launch ends
  long long* tok;            // optional [rows]
  long long* ids;            // optional: ids[r * ld]
  float* logp;               // optional: logp[r * ld]
  long ld;
  int rows, H, V;
  float inv_T;
  unsigned long long seed;
  unsigned step, row0;
  unsigned greedy_stride;     // sample_key.h's vs_row_key: 0 = no greedy rows
  const unsigned* mask;       // MASKED only: [rows][workgroups], bit c of word b = entry 32 b + c is not pickable on that row
};

// MASKED (sample_exclude.hip): an entry whose mask bit is set is treated as a -inf logit is. The workgroup needs
// word blockIdx.x of each row: one 4-byte load per half-wave, all 32 lanes the same address. The unmasked kernel is an
// instance of its own and does not read the field.
template <int NJ, int TM, bool MASKED>
__global__ __launch_bounds__(512) void vocab_sample_kernel(VocabSampleArgs a) {
  const int rows = a.rows;
  unsigned long long* best_w = a.best + (long)blockIdx.x * rows;
  unsigned long long* stat_w = a.stat + (long)blockIdx.x * rows;
  unsigned* sval_w = a.sval + (long)blockIdx.x * rows;
  vocab_front<NJ, TM>(a.h, rows, a.w, a.b, a.H, a.V, [&](int row, bool valid, float z) {
    const int ec = threadIdx.x & 31, ecol = blockIdx.x * kVocCols + ec;   // the thread's entry
    const float s = vs_scaled(z, a.inv_T);
    bool ok = ecol < a.V && s > -INFINITY;                // NaN fails the comparison
    if (MASKED) ok = ok && !(valid && ((a.mask[(long)row * gridDim.x + blockIdx.x] >> ec) & 1u));
    const float ps = ok ? s : -INFINITY;
    float bk = ok ? vs_row_key(s, a.seed, a.step, a.row0 + (unsigned)row, a.greedy_stride, (unsigned)ecol) : -INFINITY;
    int bi = ok ? ecol : kVocNone;
    float bs = ps;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {                    // the row's 32 threads are one half of a wave
      const float ov = __shfl_xor(bk, o), os = __shfl_xor(bs, o);
      const int oi = __shfl_xor(bi, o);
      if (vocab_better(ov, oi, bk, bi)) { bk = ov; bi = oi; bs = os; }
    }
    float mx, e;
    vocab_half_wave_stat(ok, ps, mx, e);
    if (ec == 0 && valid) {
      vocab_store(best_w + row, vocab_pack(bk, (unsigned)bi));
      vocab_store(stat_w + row, vocab_pack(mx, __float_as_uint(e)));
      vocab_store(sval_w + row, __float_as_uint(bs));
    }
  });
  if (!arrive_last(a.counter, gridDim.x)) return;
  // the last arriver: a wave per row, the workgroups' partials across its lanes
  const int nwg = gridDim.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int row = wave; row < rows; row += kVocWaves) {
    float bk = -INFINITY, bs = -INFINITY, M = -INFINITY;
    int bi = kVocNone;
    for (int p0 = 0; p0 < nwg; p0 += 64 * 4) {
      unsigned long long u[4], st[4];
      unsigned sv[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const long at = (long)min(p0 + 64 * q + lane, nwg - 1) * rows + row;
        u[q] = vocab_load(a.best + at);
        st[q] = vocab_load(a.stat + at);
        sv[q] = vocab_load(a.sval + at);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float v = vocab_hi(u[q]);
        const int i = (int)vocab_lo(u[q]);
        if (p0 + 64 * q + lane < nwg) {
          if (vocab_better(v, i, bk, bi)) { bk = v; bi = i; bs = __uint_as_float(sv[q]); }
          M = fmaxf(M, vocab_hi(st[q]));
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bk, o), os = __shfl_xor(bs, o);
      const int oi = __shfl_xor(bi, o);
      if (vocab_better(ov, oi, bk, bi)) { bk = ov; bi = oi; bs = os; }
      M = fmaxf(M, __shfl_xor(M, o));
    }
    float S = 0.f;           // lane l adds workgroups l, l + 64, ... in that order; then the xor tree
    for (int p0 = 0; p0 < nwg; p0 += 64 * 4) {
      unsigned long long st[4];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        st[q] = vocab_load(a.stat + (long)min(p0 + 64 * q + lane, nwg - 1) * rows + row);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float mw = vocab_hi(st[q]), sw = __uint_as_float(vocab_lo(st[q]));
        if (p0 + 64 * q + lane < nwg && mw > -INFINITY) S += sw * expf(mw - M);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) S += __shfl_xor(S, o);
    if (lane == 0) {
      const bool none = bi == kVocNone;
      const long long t = none ? 0 : bi;
      if (a.tok) a.tok[row] = t;
      if (a.ids) a.ids[(long)row * a.ld] = t;
      if (a.logp) a.logp[(long)row * a.ld] = none ? -INFINITY : bs - (M + logf(S));
    }
  }
  vocab_rearm(a.counter);
}

// one thread per row over the row's k candidates (k <= 16), in list order
__global__ __launch_bounds__(256) void sample_pick_kernel(const float* __restrict__ values, const int* __restrict__ index, int rows,
                                                          int k, int V, float inv_T, unsigned long long seed, unsigned step,
                                                          unsigned row0, unsigned greedy_stride, long long* __restrict__ tok,
                                                          long long* __restrict__ ids, float* __restrict__ logp, long ld) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= rows) return;
  float bk = -INFINITY, bs = -INFINITY, M = -INFINITY;
  int bi = kVocNone;
  for (int j = 0; j < k; ++j) {
    const int v = index[(long)row * k + j];
    const float s = vs_scaled(values[(long)row * k + j], inv_T);
    if (v < 0 || v >= V || !(s > -INFINITY)) continue;      // padding, or nothing to pick
    const float key = vs_row_key(s, seed, step, row0 + (unsigned)row, greedy_stride, (unsigned)v);
    if (vocab_better(key, v, bk, bi)) { bk = key; bi = v; bs = s; }
    M = fmaxf(M, s);
  }
  float S = 0.f;
  for (int j = 0; j < k; ++j) {
    const int v = index[(long)row * k + j];
    const float s = vs_scaled(values[(long)row * k + j], inv_T);
    if (v < 0 || v >= V || !(s > -INFINITY)) continue;
    S += expf(s - M);
  }
  const bool none = bi == kVocNone;
  const long long t = none ? 0 : bi;
  if (tok) tok[row] = t;
  if (ids) ids[(long)row * ld] = t;
  if (logp) logp[(long)row * ld] = none ? -INFINITY : bs - (M + logf(S));
}

// one workgroup per row of a logits block: thread t takes entries t, t + 256, ...; the workgroup's reductions are trees
// over LDS in a fixed order
constexpr int kSrThreads = 256;

__global__ __launch_bounds__(kSrThreads) void sample_rows_kernel(const float* __restrict__ logits, long ld_logits, int V, float inv_T,
                                                                 unsigned long long seed, unsigned step, unsigned row0,
                                                                 unsigned greedy_stride, long long* __restrict__ tok,
                                                                 long long* __restrict__ ids, float* __restrict__ logp, long ld) {
  __shared__ float sk[kSrThreads], ss[kSrThreads], sm[kSrThreads];
  __shared__ int si[kSrThreads];
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* x = logits + (long)row * ld_logits;
  float bk = -INFINITY, bs = -INFINITY, M = -INFINITY;
  int bi = kVocNone;
  for (int v = tid; v < V; v += kSrThreads) {
    const float s = vs_scaled(x[v], inv_T);
    if (!(s > -INFINITY)) continue;
    const float key = vs_row_key(s, seed, step, row0 + (unsigned)row, greedy_stride, (unsigned)v);
    if (vocab_better(key, v, bk, bi)) { bk = key; bi = v; bs = s; }
    M = fmaxf(M, s);
  }
  sk[tid] = bk; si[tid] = bi; ss[tid] = bs; sm[tid] = M;
  __syncthreads();
  for (int o = kSrThreads / 2; o > 0; o >>= 1) {
    if (tid < o) {
      if (vocab_better(sk[tid + o], si[tid + o], sk[tid], si[tid])) { sk[tid] = sk[tid + o]; si[tid] = si[tid + o]; ss[tid] = ss[tid + o]; }
      sm[tid] = fmaxf(sm[tid], sm[tid + o]);
    }
    __syncthreads();
  }
  M = sm[0];
  bi = si[0];
  bs = ss[0];
  __syncthreads();
  float S = 0.f;
  for (int v = tid; v < V; v += kSrThreads) {
    const float s = vs_scaled(x[v], inv_T);
    if (s > -INFINITY) S += expf(s - M);
  }
  sm[tid] = S;
  __syncthreads();
  for (int o = kSrThreads / 2; o > 0; o >>= 1) {
    if (tid < o) sm[tid] += sm[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    const bool none = bi == kVocNone;
    const long long t = none ? 0 : bi;
    if (tok) tok[row] = t;
    if (ids) ids[(long)row * ld] = t;
    if (logp) logp[(long)row * ld] = none ? -INFINITY : bs - (M + logf(sm[0]));
  }
}


bool vocab_sample_supported(int H) { return step_hidden_supported(H); }

float sample_uniform_host(unsigned long long seed, unsigned step, unsigned row, unsigned v) {
  return sample_uniform(seed, step, row, v);
}

// workspace: 16 bytes whose first int is the counter | best [workgroups][rows] | stat [workgroups][rows] (8-byte words) |
// sval [workgroups][rows] (4-byte words)
size_t vocab_sample_ws_bytes(int rows, int V) {
  const size_t cells = (size_t)vocab_workgroups(V) * rows;
  return 16 + 16 * cells + align16(4 * cells);
}

int vocab_sample(const float* h, const float* w, const float* b, int rows, int H, int V, float inv_T, unsigned long long seed,
                 unsigned step, unsigned row0, void* ws, long long* tok, long long* ids, float* logp, long ld,
                 hipStream_t stream, unsigned greedy_stride, const unsigned* mask) {
  CAPNET_REQUIRE(rows >= 1 && V >= 1 && vocab_sample_supported(H), "vocab_sample: rows %d, H %d, V %d", rows, H, V);
  const size_t cells = (size_t)vocab_workgroups(V) * rows;
  VocabSampleArgs a;
  a.h = h; a.w = w; a.b = b;
  a.counter = reinterpret_cast<int*>(ws);
  a.best = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(ws) + 16);
  a.stat = a.best + cells;
  a.sval = reinterpret_cast<unsigned*>(a.stat + cells);
  a.tok = tok; a.ids = ids; a.logp = logp; a.ld = ld;
  a.rows = rows; a.H = H; a.V = V;
  a.inv_T = inv_T; a.seed = seed; a.step = step; a.row0 = row0; a.greedy_stride = greedy_stride;
  a.mask = mask;
  const dim3 grid(vocab_workgroups(V)), block(64 * kVocWaves);
  dispatch_nj(H, [&](auto nj) {   // two row tiles per pass where their operands fit beside the weights
    if (mask) hipLaunchKernelGGL((vocab_sample_kernel<nj, nj <= 8 ? 2 : 1, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((vocab_sample_kernel<nj, nj <= 8 ? 2 : 1, false>), grid, block, 0, stream, a);
  });
  CAPNET_LAUNCH_CHECK();
  return kOk;
}

int sample_pick(const float* values, const int* index, int rows, int k, int V, float inv_T, unsigned long long seed,
                unsigned step, unsigned row0, long long* tok, long long* ids, float* logp, long ld, hipStream_t stream,
                unsigned greedy_stride) {
  CAPNET_REQUIRE(rows >= 1 && k >= 1 && k <= 16 && V >= 1, "sample_pick: rows %d, k %d, V %d", rows, k, V);
  hipLaunchKernelGGL(sample_pick_kernel, dim3((rows + 255) / 256), dim3(256), 0, stream, values, index, rows, k, V, inv_T, seed,
                     step, row0, greedy_stride, tok, ids, logp, ld);
  CAPNET_LAUNCH_CHECK();
  return kOk;
}

int sample_rows(const float* logits, int rows, long ld_logits, int V, float inv_T, unsigned long long seed, unsigned step,
                unsigned row0, long long* tok, long long* ids, float* logp, long ld, hipStream_t stream, unsigned greedy_stride) {
  CAPNET_REQUIRE(rows >= 1 && V >= 1 && ld_logits >= V, "sample_rows: rows %d, V %d, ld %ld", rows, V, ld_logits);
  hipLaunchKernelGGL(sample_rows_kernel, dim3(rows), dim3(kSrThreads), 0, stream, logits, ld_logits, V, inv_T, seed, step, row0,
                     greedy_stride, tok, ids, logp, ld);
  CAPNET_LAUNCH_CHECK();
  return kOk;
}

}  // namespace capnet
