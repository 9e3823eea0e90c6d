// Sampled decoding: a draw from softmax(logit / T) per row in ONE launch, the logits never in memory, and the whole
// sampling loop of a plain stack as one C call (capnet_vocab_sample, capnet_sample_pick, capnet_sample_rows,
// capnet_sample_decode).
//   z[r][v] = h[r] . W[v] + b[v]        h [rows][H], W [V][H] (nn.Linear), b [V]
//   s = z inv_T,  key = s + sample_gumbel(sample_uniform(seed, step, row0 + r, v))          (sample_rng.h)
//   tok[r] = argmax_v key (ties to the lower v),  logp[r] = s[tok] - log sum_v exp(s)
// Gumbel-max: the argmax of the noised scaled logits IS a draw from softmax(z / T), so sampling is vocab_argmax with
// counter-based noise in the epilogue; no prefix sum over the vocabulary. The noise is a pure function of (seed, step, row,
// v): the token does not depend on which workgroup arrives last, nor on how a caller splits its rows over launches (row0).
//
// Mapping: vocab_argmax_kernel's (vocab_argmax.hip) to the letter. A workgroup owns 32 vocabulary entries = two N tiles of
// the 16-row product (step_core.h) and ALL rows; its 8 waves are 2 tiles x 4 contiguous quarters of K = H; a lane loads its
// column's weights for its quarter once and keeps them while the workgroup walks the rows 16 TM at a time. The four
// K-partial tiles are summed through LDS in a fixed order and the bias is added: a row's 32 logits sit in the 32 lanes of
// half a wave. Per row the workgroup emits
//   its best (key, index) under vocab_argmax's total order (one packed 8-byte word) and that entry's s, and
//   vocab_topk's m_w = the maximum of its pickable s, s_w = sum expf(s - m_w) over them (one packed 8-byte word).
// A logit that is NaN or -inf, or lies beyond V, is not pickable: never drawn, and it adds nothing to s_w.
// Cross-workgroup: vocab_argmax_kernel's hand-off, cell by cell -- every partial an agent-scope store, every storing wave
// drained, a workgroup barrier, one lane's agent-scope atomic add on the one counter, the partials read back with
// agent-scope loads by the workgroup that arrives LAST. No workgroup waits on another. The last one merges a wave per row,
// the workgroups across its lanes: the winner under the total order; M = max m_w, S = sum s_w expf(m_w - M) with lane l
// adding workgroups l, l + 64, ... in that order and the lanes then combined by the xor tree, lse = M + logf(S): the same
// bits whoever arrives last. A row with nothing to pick yields token 0 and logp = -inf. The counter is zero before the
// first use and zero again when the launch ends. Plain vector loads and stores only.
//
// sample_pick_kernel: the same draw among the k candidates of vocab_topk's (values, index) -- top-k sampling. The noise is
// keyed by the candidate's VOCABULARY index, so k = V would draw what the full kernel draws; logp is renormalised over the
// k candidates; padding slots (-inf, -1) are never picked.
// sample_rows_kernel: the same draw from a [rows][ld] logits block in memory, one workgroup per row (the composed route).
#include "common.h"
#include "kernels.h"
#include "sample_rng.h"
#include "step_core.h"

// No contraction into fused multiply-adds anywhere in this file: s = z inv_T is a rounded product wherever it is formed, so
// the three kernels form the same key bits from the same logit, expf(s - M) of the largest s is exactly 1 and a single
// candidate's logp is exactly 0 (hipcc contracts across statements by default, and __fmul_rn is a plain product to it).
#pragma clang fp contract(off)

namespace capnet {

constexpr int kVsWaves = 8;
constexpr int kVsCols = 32;          // vocabulary entries per workgroup
constexpr int kVsNone = 0x7fffffff;

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
};

__device__ __forceinline__ bool vs_better(float v, int i, float best, int bi) {
  return v > best || (v == best && i < bi);
}

// the key of entry v of noise row `nrow`: separate roundings of the product and of the sum (see the pragma above)
__device__ __forceinline__ float vs_scaled(float z, float inv_T) { return __fmul_rn(z, inv_T); }
__device__ __forceinline__ float vs_key(float s, unsigned long long seed, unsigned step, unsigned nrow, unsigned v) {
  return __fadd_rn(s, sample_gumbel(sample_uniform(seed, step, nrow, v)));
}

template <int NJ, int TM>
__global__ __launch_bounds__(512) void vocab_sample_kernel(VocabSampleArgs a) {
  constexpr int kPass = 16 * TM;
  __shared__ float red[kVsWaves][kPass][17];
  __shared__ int s_last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lq = lane >> 4;
  const int tile = wave >> 2, ks = wave & 3;
  const int H = a.H, rows = a.rows, c0 = blockIdx.x * kVsCols;
  const int g0 = ks * NJ;                                   // this wave's k groups [g0, g0 + NJ): H = 64 NJ
  const int wcol = clamp_row(c0 + 16 * tile + li, a.V);      // entries beyond V: masked in the epilogue
  const float* wrow = a.w + (long)wcol * H + 16 * g0 + 4 * lq;
  f32x4 wv[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) wv[j] = *reinterpret_cast<const f32x4*>(wrow + 16 * j);
  // epilogue thread: (row er of a 16-row tile, entry ec of the workgroup's 32)
  const int er = tid >> 5, ec = tid & 31;
  const int ecol = c0 + ec;
  const float bias = (a.b && ecol < a.V) ? a.b[ecol] : 0.f;
  unsigned long long* best_w = a.best + (long)blockIdx.x * rows;
  unsigned long long* stat_w = a.stat + (long)blockIdx.x * rows;
  unsigned* sval_w = a.sval + (long)blockIdx.x * rows;
  for (int r0 = 0; r0 < rows; r0 += kPass) {
    f32x4 acc[TM];
#pragma unroll
    for (int m = 0; m < TM; ++m) {
      const int row = clamp_row(r0 + 16 * m + li, rows);
      const float* hrow = a.h + (long)row * H + 16 * g0 + 4 * lq;
      f32x4 av[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j) av[j] = *reinterpret_cast<const f32x4*>(hrow + 16 * j);
      acc[m] = mfma_chain<NJ>(av, wv, f32x4{0.f, 0.f, 0.f, 0.f});
    }
#pragma unroll
    for (int m = 0; m < TM; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wave][16 * m + 4 * lq + r][li] = acc[m][r];
    __syncthreads();
#pragma unroll
    for (int m = 0; m < TM; ++m) {
      const int pr = 16 * m + er, row = r0 + pr;
      const int t4 = (ec >> 4) * 4, cc = ec & 15;
      const float z = bias + red[t4][pr][cc] + red[t4 + 1][pr][cc] + red[t4 + 2][pr][cc] + red[t4 + 3][pr][cc];
      const float s = vs_scaled(z, a.inv_T);
      const bool ok = ecol < a.V && s > -INFINITY;          // NaN fails the comparison
      const float ps = ok ? s : -INFINITY;
      float bk = ok ? vs_key(s, a.seed, a.step, a.row0 + (unsigned)row, (unsigned)ecol) : -INFINITY;
      int bi = ok ? ecol : kVsNone;
      float bs = ps;
      float mx = ps;                                        // the row's 32 threads are one half of a wave
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bk, o), os = __shfl_xor(bs, o);
        const int oi = __shfl_xor(bi, o);
        if (vs_better(ov, oi, bk, bi)) { bk = ov; bi = oi; bs = os; }
        mx = fmaxf(mx, __shfl_xor(mx, o));
      }
      float e = ok ? expf(ps - mx) : 0.f;
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) e += __shfl_xor(e, o);
      if (ec == 0 && row < rows) {
        __hip_atomic_store(best_w + row, ((unsigned long long)__float_as_uint(bk) << 32) | (unsigned)bi, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(stat_w + row, ((unsigned long long)__float_as_uint(mx) << 32) | __float_as_uint(e), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(sval_w + row, __float_as_uint(bs), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    __syncthreads();   // red is rewritten by the next pass
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0)
    s_last = __hip_atomic_fetch_add(a.counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1;
  __syncthreads();
  if (!s_last) return;
  // the last arriver: a wave per row, the workgroups' partials across its lanes
  const int nwg = gridDim.x;
  for (int row = wave; row < rows; row += kVsWaves) {
    float bk = -INFINITY, bs = -INFINITY, M = -INFINITY;
    int bi = kVsNone;
    for (int p0 = 0; p0 < nwg; p0 += 64 * 4) {
      unsigned long long u[4], st[4];
      unsigned sv[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const long at = (long)min(p0 + 64 * q + lane, nwg - 1) * rows + row;
        u[q] = __hip_atomic_load(a.best + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        st[q] = __hip_atomic_load(a.stat + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sv[q] = __hip_atomic_load(a.sval + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float v = __uint_as_float((unsigned)(u[q] >> 32));
        const int i = (int)(unsigned)u[q];
        if (p0 + 64 * q + lane < nwg) {
          if (vs_better(v, i, bk, bi)) { bk = v; bi = i; bs = __uint_as_float(sv[q]); }
          M = fmaxf(M, __uint_as_float((unsigned)(st[q] >> 32)));
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bk, o), os = __shfl_xor(bs, o);
      const int oi = __shfl_xor(bi, o);
      if (vs_better(ov, oi, bk, bi)) { bk = ov; bi = oi; bs = os; }
      M = fmaxf(M, __shfl_xor(M, o));
    }
    float S = 0.f;           // lane l adds workgroups l, l + 64, ... in that order; then the xor tree
    for (int p0 = 0; p0 < nwg; p0 += 64 * 4) {
      unsigned long long st[4];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        st[q] = __hip_atomic_load(a.stat + (long)min(p0 + 64 * q + lane, nwg - 1) * rows + row, __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float mw = __uint_as_float((unsigned)(st[q] >> 32)), sw = __uint_as_float((unsigned)st[q]);
        if (p0 + 64 * q + lane < nwg && mw > -INFINITY) S += sw * expf(mw - M);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) S += __shfl_xor(S, o);
    if (lane == 0) {
      const bool none = bi == kVsNone;
      const long long t = none ? 0 : bi;
      if (a.tok) a.tok[row] = t;
      if (a.ids) a.ids[(long)row * a.ld] = t;
      if (a.logp) a.logp[(long)row * a.ld] = none ? -INFINITY : bs - (M + logf(S));
    }
  }
  if (tid == 0) __hip_atomic_store(a.counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one thread per row over the row's k candidates (k <= 16), in list order
__global__ __launch_bounds__(256) void sample_pick_kernel(const float* __restrict__ values, const int* __restrict__ index, int rows,
                                                          int k, int V, float inv_T, unsigned long long seed, unsigned step,
                                                          unsigned row0, long long* __restrict__ tok, long long* __restrict__ ids,
                                                          float* __restrict__ logp, long ld) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= rows) return;
  float bk = -INFINITY, bs = -INFINITY, M = -INFINITY;
  int bi = kVsNone;
  for (int j = 0; j < k; ++j) {
    const int v = index[(long)row * k + j];
    const float s = vs_scaled(values[(long)row * k + j], inv_T);
    if (v < 0 || v >= V || !(s > -INFINITY)) continue;      // padding, or nothing to pick
    const float key = vs_key(s, seed, step, row0 + (unsigned)row, (unsigned)v);
    if (vs_better(key, v, bk, bi)) { bk = key; bi = v; bs = s; }
    M = fmaxf(M, s);
  }
  float S = 0.f;
  for (int j = 0; j < k; ++j) {
    const int v = index[(long)row * k + j];
    const float s = vs_scaled(values[(long)row * k + j], inv_T);
    if (v < 0 || v >= V || !(s > -INFINITY)) continue;
    S += expf(s - M);
  }
  const bool none = bi == kVsNone;
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
                                                                 long long* __restrict__ tok, long long* __restrict__ ids,
                                                                 float* __restrict__ logp, long ld) {
  __shared__ float sk[kSrThreads], ss[kSrThreads], sm[kSrThreads];
  __shared__ int si[kSrThreads];
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* x = logits + (long)row * ld_logits;
  float bk = -INFINITY, bs = -INFINITY, M = -INFINITY;
  int bi = kVsNone;
  for (int v = tid; v < V; v += kSrThreads) {
    const float s = vs_scaled(x[v], inv_T);
    if (!(s > -INFINITY)) continue;
    const float key = vs_key(s, seed, step, row0 + (unsigned)row, (unsigned)v);
    if (vs_better(key, v, bk, bi)) { bk = key; bi = v; bs = s; }
    M = fmaxf(M, s);
  }
  sk[tid] = bk; si[tid] = bi; ss[tid] = bs; sm[tid] = M;
  __syncthreads();
  for (int o = kSrThreads / 2; o > 0; o >>= 1) {
    if (tid < o) {
      if (vs_better(sk[tid + o], si[tid + o], sk[tid], si[tid])) { sk[tid] = sk[tid + o]; si[tid] = si[tid + o]; ss[tid] = ss[tid + o]; }
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
    const bool none = bi == kVsNone;
    const long long t = none ? 0 : bi;
    if (tok) tok[row] = t;
    if (ids) ids[(long)row * ld] = t;
    if (logp) logp[(long)row * ld] = none ? -INFINITY : bs - (M + logf(sm[0]));
  }
}

static int vs_workgroups(int V) { return (V + kVsCols - 1) / kVsCols; }
static size_t vs_align(size_t n) { return (n + 15) / 16 * 16; }

bool vocab_sample_supported(int H) { return step_hidden_supported(H); }

float sample_uniform_host(unsigned long long seed, unsigned step, unsigned row, unsigned v) {
  return sample_uniform(seed, step, row, v);
}

// workspace: 16 bytes whose first int is the counter | best [workgroups][rows] | stat [workgroups][rows] (8-byte words) |
// sval [workgroups][rows] (4-byte words)
size_t vocab_sample_ws_bytes(int rows, int V) {
  const size_t cells = (size_t)vs_workgroups(V) * rows;
  return 16 + 16 * cells + vs_align(4 * cells);
}

int vocab_sample(const float* h, const float* w, const float* b, int rows, int H, int V, float inv_T, unsigned long long seed,
                 unsigned step, unsigned row0, void* ws, long long* tok, long long* ids, float* logp, long ld,
                 hipStream_t stream) {
  CAPNET_REQUIRE(rows >= 1 && V >= 1 && vocab_sample_supported(H), "vocab_sample: rows %d, H %d, V %d", rows, H, V);
  const size_t cells = (size_t)vs_workgroups(V) * rows;
  VocabSampleArgs a;
  a.h = h; a.w = w; a.b = b;
  a.counter = reinterpret_cast<int*>(ws);
  a.best = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(ws) + 16);
  a.stat = a.best + cells;
  a.sval = reinterpret_cast<unsigned*>(a.stat + cells);
  a.tok = tok; a.ids = ids; a.logp = logp; a.ld = ld;
  a.rows = rows; a.H = H; a.V = V;
  a.inv_T = inv_T; a.seed = seed; a.step = step; a.row0 = row0;
  const dim3 grid(vs_workgroups(V)), block(64 * kVsWaves);
  dispatch_nj(H, [&](auto nj) {   // two row tiles per pass where their operands fit beside the weights
    hipLaunchKernelGGL((vocab_sample_kernel<nj, nj <= 8 ? 2 : 1>), grid, block, 0, stream, a);
  });
  CAPNET_LAUNCH_CHECK();
  return kOk;
}

int sample_pick(const float* values, const int* index, int rows, int k, int V, float inv_T, unsigned long long seed,
                unsigned step, unsigned row0, long long* tok, long long* ids, float* logp, long ld, hipStream_t stream) {
  CAPNET_REQUIRE(rows >= 1 && k >= 1 && k <= 16 && V >= 1, "sample_pick: rows %d, k %d, V %d", rows, k, V);
  hipLaunchKernelGGL(sample_pick_kernel, dim3((rows + 255) / 256), dim3(256), 0, stream, values, index, rows, k, V, inv_T, seed,
                     step, row0, tok, ids, logp, ld);
  CAPNET_LAUNCH_CHECK();
  return kOk;
}

int sample_rows(const float* logits, int rows, long ld_logits, int V, float inv_T, unsigned long long seed, unsigned step,
                unsigned row0, long long* tok, long long* ids, float* logp, long ld, hipStream_t stream) {
  CAPNET_REQUIRE(rows >= 1 && V >= 1 && ld_logits >= V, "sample_rows: rows %d, V %d, ld %ld", rows, V, ld_logits);
  hipLaunchKernelGGL(sample_rows_kernel, dim3(rows), dim3(kSrThreads), 0, stream, logits, ld_logits, V, inv_T, seed, step, row0, tok,
                     ids, logp, ld);
  CAPNET_LAUNCH_CHECK();
  return kOk;
}

// ---- the whole sampling loop of a plain stack: steps x (one decode-step launch per layer + the draw) -- lstm_greedy_decode's
// loop with the cell kind passed through; the draw is vocab_sample (top_k == 0) or vocab_topk + sample_pick (top_k > 0).
// The loop does not look at an end token: it runs `steps` steps and the host truncates.
// ws: [state A | state B] ([rows][2L][H] each) | h_top [rows][H] | tok int64 [rows] | top_k == 0: vocab_sample's workspace;
// else values f32 [rows][k] | index int32 [rows][k] | lse f32 [rows] | vocab_topk's workspace
size_t sample_decode_ws_bytes(int nlayers, int rows, int H, int V, int top_k) {
  const size_t st = vs_align((size_t)rows * 2 * nlayers * H * sizeof(float));
  size_t n = 2 * st + vs_align((size_t)rows * H * sizeof(float)) + vs_align((size_t)rows * 8);
  if (top_k == 0) return n + vocab_sample_ws_bytes(rows, V);
  const size_t tk = vocab_topk_ws_bytes(rows, top_k, V);
  if (!tk) return 0;
  return n + 2 * vs_align((size_t)rows * top_k * 4) + vs_align((size_t)rows * 4) + tk;
}

// the loop of the one-call samplers: step_fn(t, tokens, state_in, state_out, h_top) is the decode step of step t
template <class Step>
static int sample_loop(int nlayers, int rows, int H, int V, int steps, const long long* start_tokens, const float* Cw,
                       const float* Cb, const float* state0, float inv_T, int top_k, unsigned long long seed, void* ws,
                       long long* ids, float* logp, float* state_out, hipStream_t s, Step&& step_fn) {
  const size_t st_bytes = (size_t)rows * 2 * nlayers * H * sizeof(float), st = vs_align(st_bytes);
  char* p = reinterpret_cast<char*>(ws);
  float* state[2] = {reinterpret_cast<float*>(p), reinterpret_cast<float*>(p + st)};
  p += 2 * st;
  float* h_top = reinterpret_cast<float*>(p);
  p += vs_align((size_t)rows * H * sizeof(float));
  long long* tok = reinterpret_cast<long long*>(p);
  p += vs_align((size_t)rows * 8);
  float* tk_values = nullptr;
  float* tk_lse = nullptr;
  int* tk_index = nullptr;
  if (top_k > 0) {
    tk_values = reinterpret_cast<float*>(p);
    p += vs_align((size_t)rows * top_k * 4);
    tk_index = reinterpret_cast<int*>(p);
    p += vs_align((size_t)rows * top_k * 4);
    tk_lse = reinterpret_cast<float*>(p);
    p += vs_align((size_t)rows * 4);
  }
  void* draw_ws = p;
  if (state0) CAPNET_HIP_CHECK(hipMemcpyAsync(state[0], state0, st_bytes, hipMemcpyDeviceToDevice, s));
  else CAPNET_HIP_CHECK(hipMemsetAsync(state[0], 0, st_bytes, s));
  if (start_tokens) CAPNET_HIP_CHECK(hipMemcpyAsync(tok, start_tokens, (size_t)rows * 8, hipMemcpyDeviceToDevice, s));
  CAPNET_HIP_CHECK(hipMemsetAsync(draw_ws, 0, 16, s));    // the arrival counter of vocab_sample or of vocab_topk
  for (int t = 0; t < steps; ++t) {
    int rc = step_fn(t, tok, state[t & 1], state[(t + 1) & 1], h_top);
    if (rc == kOk && top_k == 0)
      rc = vocab_sample(h_top, Cw, Cb, rows, H, V, inv_T, seed, (unsigned)t, 0, draw_ws, tok, ids + t, logp + t, steps, s);
    if (rc == kOk && top_k > 0) {
      rc = vocab_topk(h_top, Cw, Cb, rows, H, V, top_k, draw_ws, tk_values, tk_index, tk_lse, s);
      if (rc == kOk) rc = sample_pick(tk_values, tk_index, rows, top_k, V, inv_T, seed, (unsigned)t, 0, tok, ids + t, logp + t, steps, s);
    }
    if (rc != kOk) return rc;
  }
  if (state_out) CAPNET_HIP_CHECK(hipMemcpyAsync(state_out, state[steps & 1], st_bytes, hipMemcpyDeviceToDevice, s));
  return kOk;
}

int sample_decode(int cell, int nlayers, int rows, int E, int H, int V, int steps, const float* first_inputs,
                  const long long* start_tokens, const float* emb, const float* const* wcat, const float* const* beff,
                  const float* Cw, const float* Cb, const float* state0, float inv_T, int top_k, unsigned long long seed, void* ws,
                  long long* ids, float* logp, float* state_out, int* err_flag, hipStream_t s) {
  return sample_loop(nlayers, rows, H, V, steps, start_tokens, Cw, Cb, state0, inv_T, top_k, seed, ws, ids, logp, state_out, s,
                     [&](int t, const long long* tok, const float* sin, float* sout, float* h_top) {
                       const bool given = t == 0 && first_inputs;     // step 0 on the caller's rows
                       return stacked_decode_step(cell, nlayers, rows, E, H, V, given ? nullptr : tok, given ? first_inputs : emb,
                                                  wcat, beff, sin, sout, h_top, err_flag, s);
                     });
}

// ---- the same loop for the attention decoders: n images x m samples each, the step att_decode_step with k = m and every
// row continuing from itself (parent_rows null at every step), so an image's maps are read once per step for all its
// samples. No beam bookkeeping.
// ws: sample_decode's layout at n m rows, then att_decode_step's block (z | xa | escore)
size_t att_sample_decode_ws_bytes(int nlayers, int n, int m, int P, int A, int C, int E, int H, int V, int top_k) {
  if (n < 1 || m < 1 || (long)n * m >= (1L << 24)) return 0;
  const size_t base = sample_decode_ws_bytes(nlayers, n * m, H, V, top_k), step = att_decode_step_ws_bytes(n, m, P, A, C, E);
  return base && step ? vs_align(base) + vs_align(step) : 0;
}

int att_sample_decode(int cell, int nlayers, int n, int m, int P, int A, int C, int E, int H, int V, int steps,
                      const long long* start_tokens, const float* att1, const float* feat, const float* emb, const float* wz,
                      const float* bz, const float* wf, const float* bf, const float* const* wcat, const float* const* beff,
                      const float* Cw, const float* Cb, const float* state0, float inv_T, int top_k, unsigned long long seed,
                      void* ws, float* slab, size_t slab_floats, long long* ids, float* logp, float* state_out, int* err_flag,
                      hipStream_t s) {
  const int rows = n * m;
  void* step_ws = reinterpret_cast<char*>(ws) + vs_align(sample_decode_ws_bytes(nlayers, rows, H, V, top_k));
  return sample_loop(nlayers, rows, H, V, steps, start_tokens, Cw, Cb, state0, inv_T, top_k, seed, ws, ids, logp, state_out, s,
                     [&](int, const long long* tok, const float* sin, float* sout, float* h_top) {
                       return att_decode_step(cell, nlayers, n, m, P, A, C, E, H, V, att1, feat, tok, emb, wz, bz, wf, bf, wcat, beff,
                                              sin, nullptr, sout, h_top, step_ws, slab, slab_floats, err_flag, s);
                     });
}

}  // namespace capnet
