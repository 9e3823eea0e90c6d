// Greedy decoding of capnet.seq2seq (seq2seq/model.py:100-122, 193-217): the vocabulary projection and its argmax in ONE
// launch, without the logits ever reaching memory, and the whole `sample` loop as one C call.
//   tok[r] = first argmax_v (h[r] . W[v] + b[v])        h [rows][H], W [V][H] (nn.Linear), b [V]
//
// Mapping (the arrangement of lstm_decode_step.hip): a workgroup owns 32 vocabulary entries = two N tiles of
// the 16-row product (step_core.h) and ALL rows. Its 8 waves are 2 tiles x 4 contiguous quarters of K = H; a lane loads its column's
// weights for its quarter once (NJ f32x4 registers: the projection crosses the memory system once per launch) and keeps
// them while the workgroup walks the rows 16 TM at a time. The four K-partial tiles are summed through LDS in a fixed order,
// the bias is added, and 32 threads per row reduce (value, index) with a strict comparison, ties to the lower index.
// Cross-workgroup: each workgroup writes one packed (value, index) word per row; the workgroup that arrives LAST at the one
// counter (gemm_rows16_kernel's hand-off in gemm_f32.hip, cell by cell: every partial an 8-byte agent-scope store, every
// storing wave drained, a workgroup barrier, one lane's agent-scope atomic add, the partials read back with agent-scope
// loads) reduces them per row -- the winner does not depend on who was last, the comparison is a total order on
// (value, index) -- writes the int64 token where the next step's layer-0 launch gathers its embedding row (and into the
// ids matrix), and puts the counter back to zero. No workgroup waits on another. Plain vector loads and stores only.
// NaN and -inf logits are never picked (strict `>` against -inf, as argmax_rows_kernel); a row with nothing to pick
// yields 0.
// Weight groups (every emotion of capnet.seq2seq at once: capnet_vocab_argmax_groups, capnet_lstm_greedy_decode_groups): the
// grid is (ceil(V / 32), G), rows are group-major, and workgroup (., g) projects rows [g rpg, (g + 1) rpg) on w[g] / b[g]
// -- one pointer per group held by value in the argument struct and picked by blockIdx.y, a scalar load from the kernel
// arguments; no projection is copied. It writes its partials to group g's block and arrives at group g's OWN counter (16
// bytes apart), where arrivals are counted against gridDim.x: group g's last arriver reduces group g's rows, writes their
// tokens and re-arms that counter only. The groups never meet. G = 1 is the kernel as it was: the same grid, the same
// addresses, the same bits.
#include "common.h"
#include "kernels.h"
#include "step_core.h"

namespace capnet {

constexpr int kVaWaves = 8;
constexpr int kVaCols = 32;          // vocabulary entries per workgroup
constexpr int kVaNone = 0x7fffffff;

constexpr int kVaMaxGroups = 8;      // weight groups of one launch

struct VocabArgmaxArgs {
  const float* h;            // [rows][H], group-major
  unsigned long long* part;  // [groups][workgroups][rpg]: (value bits << 32) | index
  int* counter;              // group g's at counter + 4 g; zero before the first use, zero again when the launch ends
  long long* tok;            // optional [rows]
  long long* ids;            // optional: ids[r * ld_ids]
  long ld_ids;
  int rpg, H, V;             // rows per group: workgroup (., g) owns rows [g rpg, (g + 1) rpg)
  const float* w[kVaMaxGroups];   // [V][H] of group g
  const float* b[kVaMaxGroups];   // [V] of group g, or null
};

__device__ __forceinline__ bool va_better(float v, int i, float best, int bi) {
  return v > best || (v == best && i < bi);
}

template <int NJ, int TM>
__global__ __launch_bounds__(512) void vocab_argmax_kernel(VocabArgmaxArgs a) {
  constexpr int kPass = 16 * TM;
  __shared__ float red[kVaWaves][kPass][17];
  __shared__ int s_last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lq = lane >> 4;
  const int tile = wave >> 2, ks = wave & 3;
  const int H = a.H, c0 = blockIdx.x * kVaCols;
  const int g0 = ks * NJ;                                   // this wave's k groups [g0, g0 + NJ): H = 64 NJ
  const int wcol = clamp_row(c0 + 16 * tile + li, a.V);      // entries beyond V: masked in the epilogue
  const int grp = blockIdx.y, rbeg = grp * a.rpg, rend = rbeg + a.rpg;   // this group's rows; one group: [0, rows)
  const float* bg = a.b[grp];
  const float* wrow = a.w[grp] + (long)wcol * H + 16 * g0 + 4 * lq;
  f32x4 wv[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) wv[j] = *reinterpret_cast<const f32x4*>(wrow + 16 * j);
  // epilogue thread: (row er of a 16-row tile, entry ec of the workgroup's 32)
  const int er = tid >> 5, ec = tid & 31;
  const int ecol = c0 + ec;
  const float bias = (bg && ecol < a.V) ? bg[ecol] : 0.f;
  unsigned long long* gpart = a.part + (long)grp * gridDim.x * a.rpg;    // the group's block, [workgroups][rpg]
  unsigned long long* part = gpart + (long)blockIdx.x * a.rpg;
  for (int r0 = rbeg; r0 < rend; r0 += kPass) {
    f32x4 acc[TM];
#pragma unroll
    for (int m = 0; m < TM; ++m) {
      const int row = clamp_row(r0 + 16 * m + li, rend);
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
      const float v = bias + red[t4][pr][cc] + red[t4 + 1][pr][cc] + red[t4 + 2][pr][cc] + red[t4 + 3][pr][cc];
      float best = -INFINITY;
      int bi = kVaNone;
      if (ecol < a.V && v > best) { best = v; bi = ecol; }
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) {                    // the row's 32 threads are one half of a wave
        const float ov = __shfl_xor(best, o);
        const int oi = __shfl_xor(bi, o);
        if (va_better(ov, oi, best, bi)) { best = ov; bi = oi; }
      }
      if (ec == 0 && row < rend)
        __hip_atomic_store(part + (row - rbeg), ((unsigned long long)__float_as_uint(best) << 32) | (unsigned)bi, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();   // red is rewritten by the next pass
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0)
    s_last = __hip_atomic_fetch_add(a.counter + 4 * grp, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1;
  __syncthreads();
  if (!s_last) return;
  // the group's last arriver: a wave per row of the group, the workgroups' partials across its lanes
  const int nwg = gridDim.x;
  for (int row = rbeg + wave; row < rend; row += kVaWaves) {
    float best = -INFINITY;
    int bi = kVaNone;
    for (int p0 = 0; p0 < nwg; p0 += 64 * 4) {
      unsigned long long u[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int p = min(p0 + 64 * q + lane, nwg - 1);
        u[q] = __hip_atomic_load(gpart + (long)p * a.rpg + (row - rbeg), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float v = __uint_as_float((unsigned)(u[q] >> 32));
        const int i = (int)(unsigned)u[q];
        if (p0 + 64 * q + lane < nwg && va_better(v, i, best, bi)) { best = v; bi = i; }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o);
      const int oi = __shfl_xor(bi, o);
      if (va_better(ov, oi, best, bi)) { best = ov; bi = oi; }
    }
    if (lane == 0) {
      const long long t = bi == kVaNone ? 0 : bi;
      if (a.tok) a.tok[row] = t;
      if (a.ids) a.ids[(long)row * a.ld_ids] = t;
    }
  }
  if (tid == 0) __hip_atomic_store(a.counter + 4 * grp, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

static int va_workgroups(int V) { return (V + kVaCols - 1) / kVaCols; }

bool vocab_argmax_supported(int H) { return step_hidden_supported(H); }

// workspace: per group 16 bytes whose first int is the group's counter, then one 8-byte partial per group, workgroup and row
size_t vocab_argmax_groups_ws_bytes(int groups, int rpg, int V) {
  return 16 * (size_t)groups + (size_t)groups * va_workgroups(V) * rpg * 8;
}
size_t vocab_argmax_ws_bytes(int rows, int V) { return vocab_argmax_groups_ws_bytes(1, rows, V); }

int vocab_argmax(const float* h, const float* w, const float* b, int rows, int H, int V, void* ws, long long* tok,
                 long long* ids, long ld_ids, hipStream_t stream) {
  return vocab_argmax_groups(h, &w, b ? &b : nullptr, 1, rows, H, V, ws, tok, ids, ld_ids, stream);
}

int vocab_argmax_groups(const float* h, const float* const* w, const float* const* b, int groups, int rpg, int H, int V,
                        void* ws, long long* tok, long long* ids, long ld_ids, hipStream_t stream) {
  CAPNET_REQUIRE(groups >= 1 && groups <= kVaMaxGroups && rpg >= 1, "vocab_argmax: %d groups of %d rows", groups, rpg);
  VocabArgmaxArgs a;
  a.h = h;
  for (int g = 0; g < kVaMaxGroups; ++g) {
    a.w[g] = w[g < groups ? g : 0];
    a.b[g] = b ? b[g < groups ? g : 0] : nullptr;
  }
  a.counter = reinterpret_cast<int*>(ws);
  a.part = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(ws) + 16 * (size_t)groups);
  a.tok = tok; a.ids = ids; a.ld_ids = ld_ids;
  a.rpg = rpg; a.H = H; a.V = V;
  const dim3 grid(va_workgroups(V), groups), block(64 * kVaWaves);
  dispatch_nj(H, [&](auto nj) {   // two row tiles per pass where their operands fit beside the weights
    hipLaunchKernelGGL((vocab_argmax_kernel<nj, nj <= 8 ? 2 : 1>), grid, block, 0, stream, a);
  });
  CAPNET_LAUNCH_CHECK();
  return kOk;
}

// ---- the whole greedy `sample`: steps x (one decode-step launch per layer + one vocab_argmax launch) ------------------
// ws: [state A | state B] ([rows][2L][H] each) | h_top [rows][H] | tok int64 [rows] | vocab_argmax's workspace
static size_t gd_align(size_t n) { return (n + 15) / 16 * 16; }

size_t lstm_greedy_decode_groups_ws_bytes(int nlayers, int groups, int rpg, int H, int V) {
  const size_t rows = (size_t)groups * rpg, st = gd_align(rows * 2 * nlayers * H * sizeof(float));
  return 2 * st + gd_align(rows * H * sizeof(float)) + gd_align(rows * 8) + vocab_argmax_groups_ws_bytes(groups, rpg, V);
}

size_t lstm_greedy_decode_ws_bytes(int nlayers, int rows, int H, int V) {
  return lstm_greedy_decode_groups_ws_bytes(nlayers, 1, rows, H, V);
}

int lstm_greedy_decode(int nlayers, int rows, int E, int H, int V, int steps, const float* features,
                       const long long* start_tokens, const float* emb, const float* const* wcat,
                       const float* const* beff, const float* Cw, const float* Cb, const float* state0, void* ws,
                       long long* ids, float* state_out, int* err_flag, hipStream_t s) {
  return lstm_greedy_decode_groups(nlayers, 1, rows, E, H, V, steps, features, start_tokens, &emb, wcat, beff, &Cw, &Cb, state0,
                                   ws, ids, state_out, err_flag, s);
}

// group g's rows [g rpg, (g + 1) rpg) decode on emb[g], wcat[l] + g 4H (kin + H), beff[l] + g 4H, Cw[g], Cb[g]
int lstm_greedy_decode_groups(int nlayers, int groups, int rpg, int E, int H, int V, int steps, const float* features,
                              const long long* start_tokens, const float* const* emb, const float* const* wcat,
                              const float* const* beff, const float* const* Cw, const float* const* Cb, const float* state0,
                              void* ws, long long* ids, float* state_out, int* err_flag, hipStream_t s) {
  const int rows = groups * rpg;
  const size_t st_bytes = (size_t)rows * 2 * nlayers * H * sizeof(float), st = gd_align(st_bytes);
  char* p = reinterpret_cast<char*>(ws);
  float* state[2] = {reinterpret_cast<float*>(p), reinterpret_cast<float*>(p + st)};
  p += 2 * st;
  float* h_top = reinterpret_cast<float*>(p);
  p += gd_align((size_t)rows * H * sizeof(float));
  long long* tok = reinterpret_cast<long long*>(p);
  p += gd_align((size_t)rows * 8);
  void* va_ws = p;
  if (state0) CAPNET_HIP_CHECK(hipMemcpyAsync(state[0], state0, st_bytes, hipMemcpyDeviceToDevice, s));
  else CAPNET_HIP_CHECK(hipMemsetAsync(state[0], 0, st_bytes, s));
  if (start_tokens) CAPNET_HIP_CHECK(hipMemcpyAsync(tok, start_tokens, (size_t)rows * 8, hipMemcpyDeviceToDevice, s));
  CAPNET_HIP_CHECK(hipMemsetAsync(va_ws, 0, 16 * (size_t)groups, s));
  for (int t = 0; t < steps; ++t) {
    const bool feat = t == 0 && features;    // (one group only: capnet_lstm_greedy_decode)
    int rc = stacked_decode_step(kCellLSTM, nlayers, rows, E, H, V, feat ? nullptr : tok, feat ? features : emb[0], wcat, beff,
                                 state[t & 1], state[(t + 1) & 1], h_top, err_flag, s, nullptr, groups, feat ? nullptr : emb);
    if (rc == kOk) rc = vocab_argmax_groups(h_top, Cw, Cb, groups, rpg, H, V, va_ws, tok, ids + t, steps, s);
    if (rc != kOk) return rc;
  }
  CAPNET_HIP_CHECK(hipMemcpyAsync(state_out, state[steps & 1], st_bytes, hipMemcpyDeviceToDevice, s));
  return kOk;
}

// ---- the whole beam search of a plain stack: steps x (one gathered decode-step launch per layer + the vocabulary
// projection + one beam_advance launch), then beam_finish -- capnet.beam.beam_search_device's loop without its host side
// ws: [state A | state B] ([n k][2L][H] each) | h_top [n k][H] | logits [n k][V] | words A | words B | parent_rows (int64
// [n k] each) | the beam_state_bytes block; every part starts 16-B aligned. fused (capnet_lstm_beam_decode on
// capnet_vocab_topk): no logits block; in its place values f32 [n k][k] | index int32 [n k][k] | lse f32 [n k] |
// vocab_topk's workspace
struct BeamDecodeWs {
  size_t state, h_top, logits, words, parent, beam, total;   // byte offsets (state B at state + (h_top - state) / 2)
  size_t tk_values, tk_index, tk_lse, tk_ws;                 // fused only
};
static BeamDecodeWs beam_decode_layout(int nlayers, int n, int k, int H, int V, int max_steps, bool fused = false,
                                       int groups = 1) {   // n: all sentences, groups x sentences per group
  const size_t nk = (size_t)n * k;
  BeamDecodeWs w;
  w.state = 0;
  w.h_top = 2 * gd_align(nk * 2 * nlayers * H * sizeof(float));
  w.logits = w.h_top + gd_align(nk * H * sizeof(float));
  w.words = w.logits + (fused ? 0 : gd_align(nk * V * sizeof(float)));
  w.tk_values = w.tk_index = w.tk_lse = w.tk_ws = 0;
  if (fused) {
    w.tk_values = w.words;
    w.tk_index = w.tk_values + gd_align(nk * k * sizeof(float));
    w.tk_lse = w.tk_index + gd_align(nk * k * sizeof(int));
    w.tk_ws = w.tk_lse + gd_align(nk * sizeof(float));
    w.words = w.tk_ws + gd_align(vocab_topk_groups_ws_bytes(groups, (int)nk / groups, k, V));
  }
  w.parent = w.words + 2 * gd_align(nk * 8);
  w.beam = w.parent + gd_align(nk * 8);
  w.total = w.beam + gd_align(beam_state_bytes(n, k, max_steps));
  return w;
}

size_t beam_decode_ws_bytes(int nlayers, int n, int k, int H, int V, int max_steps) {
  if (nlayers < 1 || nlayers > 8 || n < 1 || H < 1 || V < 1 || !beam_state_bytes(n, k, max_steps)) return 0;
  return beam_decode_layout(nlayers, n, k, H, V, max_steps).total;
}

// the loop of the one-call searches: step(tokens, parent rows or null, state_in, state_out, h_top) is the decode step
// (parent rows null: step 1). fused: the projection and the selection as vocab_topk + beam_advance_topk, no logits
// block and no slab; else sgemm_splitk on the slab + beam_advance. Cwg / Cbg (capnet_lstm_beam_decode_groups): n = groups x
// sentences per group, group-major, and group g's rows are projected on Cwg[g] / Cbg[g] -- fused, one vocab_topk_groups
// launch; else one sgemm_splitk per group into the group's row block of the logits, one after the other on the one slab
template <class Step>
static int beam_loop(int nlayers, int n, int k, int H, int V, int max_steps, long long start_token, long long end_token,
                     const float* Cw, const float* Cb, const float* state0, void* ws, float* slab, size_t slab_floats,
                     int poll_every, long long* seqs, int* lengths, int* steps_run, hipStream_t s, Step&& step_fn,
                     bool fused = false, int groups = 1, const float* const* Cwg = nullptr, const float* const* Cbg = nullptr,
                     void* trace = nullptr, int* trace_rows = nullptr) {   // (the row trace: beam_advance's, logits form only)
  const int nk = n * k, rpg = nk / groups;
  const BeamDecodeWs w = beam_decode_layout(nlayers, n, k, H, V, max_steps, fused, groups);
  const size_t st_bytes = (size_t)nk * 2 * nlayers * H * sizeof(float);
  char* p = reinterpret_cast<char*>(ws);
  float* state[2] = {reinterpret_cast<float*>(p + w.state), reinterpret_cast<float*>(p + w.state + w.h_top / 2)};
  float* h_top = reinterpret_cast<float*>(p + w.h_top);
  float* logits = reinterpret_cast<float*>(p + w.logits);
  float* tk_values = reinterpret_cast<float*>(p + w.tk_values);
  int* tk_index = reinterpret_cast<int*>(p + w.tk_index);
  float* tk_lse = reinterpret_cast<float*>(p + w.tk_lse);
  void* tk_ws = p + w.tk_ws;
  long long* words[2] = {reinterpret_cast<long long*>(p + w.words),
                         reinterpret_cast<long long*>(p + w.words + (w.parent - w.words) / 2)};
  long long* parent = reinterpret_cast<long long*>(p + w.parent);
  void* beam = p + w.beam;
  const int* live_total = nullptr;
  if (int rc = beam_live(beam, n, k, max_steps, &live_total, nullptr, nullptr)) return rc;
  if (state0) CAPNET_HIP_CHECK(hipMemcpyAsync(state[0], state0, st_bytes, hipMemcpyDeviceToDevice, s));
  else CAPNET_HIP_CHECK(hipMemsetAsync(state[0], 0, st_bytes, s));
  if (int rc = beam_init(beam, n, k, max_steps, start_token, words[0], s)) return rc;
  if (fused) CAPNET_HIP_CHECK(hipMemsetAsync(tk_ws, 0, 16 * (size_t)groups, s));   // vocab_topk's counters, one per group
  int issued = 0;
  for (int step = 1; step <= max_steps; ++step) {
    // step 1: every beam is at its own (initial) row; afterwards the rows the previous beam_advance chose
    int rc = step_fn(words[(step - 1) & 1], step == 1 ? nullptr : parent, state[(step - 1) & 1], state[step & 1], h_top);
    if (fused) {
      if (rc == kOk)
        rc = Cwg ? vocab_topk_groups(h_top, Cwg, Cbg, groups, rpg, H, V, k, tk_ws, tk_values, tk_index, tk_lse, s)
                 : vocab_topk(h_top, Cw, Cb, nk, H, V, k, tk_ws, tk_values, tk_index, tk_lse, s);
      if (rc == kOk)
        rc = beam_advance_topk(beam, tk_values, tk_index, tk_lse, V, n, k, max_steps, step, end_token, words[step & 1], parent, s);
    } else {
      for (int g = 0; Cwg && g < groups && rc == kOk; ++g)
        rc = sgemm_splitk(false, true, rpg, V, H, h_top + (size_t)g * rpg * H, H, Cwg[g], H, logits + (size_t)g * rpg * V, V,
                          Cbg ? Cbg[g] : nullptr, 0, slab, slab_floats, s);
      if (rc == kOk && !Cwg) rc = sgemm_splitk(false, true, nk, V, H, h_top, H, Cw, H, logits, V, Cb, 0, slab, slab_floats, s);
      if (rc == kOk) rc = beam_advance(beam, logits, V, V, n, k, max_steps, step, end_token, words[step & 1], parent, s, trace);
    }
    if (rc != kOk) return rc;
    issued = step;
    if (poll_every > 0 && step % poll_every == 0 && step < max_steps) {
      int live = 0;
      CAPNET_HIP_CHECK(hipMemcpyAsync(&live, live_total, sizeof(int), hipMemcpyDeviceToHost, s));
      CAPNET_HIP_CHECK(hipStreamSynchronize(s));
      if (!live) break;
    }
  }
  if (steps_run) *steps_run = issued;
  return beam_finish(beam, n, k, max_steps, end_token, seqs, lengths, s, trace, trace_rows);
}

int beam_decode(int cell, int nlayers, int n, int k, int E, int H, int V, int max_steps, long long start_token,
                long long end_token, const float* emb, const float* const* wcat, const float* const* beff, const float* Cw,
                const float* Cb, const float* state0, void* ws, float* slab, size_t slab_floats, int poll_every,
                long long* seqs, int* lengths, int* steps_run, int* err_flag, hipStream_t s, int groups) {
  n *= groups;   // beam groups: weight groups x images, group-major
  return beam_loop(nlayers, n, k, H, V, max_steps, start_token, end_token, Cw, Cb, state0, ws, slab, slab_floats, poll_every, seqs,
                   lengths, steps_run, s,
                   [&](const long long* tok, const long long* parent, const float* sin, float* sout, float* h_top) {
                     return stacked_decode_step(cell, nlayers, n * k, E, H, V, tok, emb, wcat, beff, sin, sout, h_top, err_flag, s,
                                                parent, groups);
                   });
}

// ---- capnet.seq2seq's beam search: the same loop from a given state, step 1 on given inputs (EncoderRNN's feature
// column) when first_inputs is set, the projection and selection fused (vocab_topk.hip) or as beam_decode's ----
size_t lstm_beam_decode_ws_bytes(int nlayers, int n, int k, int H, int V, int max_steps, int fused_topk) {
  if (nlayers < 1 || nlayers > 8 || n < 1 || H < 1 || V < 1 || k > V || !beam_state_bytes(n, k, max_steps)) return 0;
  if ((long)n * k >= (1L << 24) || (fused_topk && !vocab_topk_supported(H, k, V))) return 0;
  return beam_decode_layout(nlayers, n, k, H, V, max_steps, fused_topk != 0).total;
}

int lstm_beam_decode(int cell, int nlayers, int n, int k, int E, int H, int V, int max_steps, long long start_token,
                     long long end_token, const float* first_inputs, const float* emb, const float* const* wcat,
                     const float* const* beff, const float* Cw, const float* Cb, const float* state0, void* ws, float* slab,
                     size_t slab_floats, int fused_topk, int poll_every, long long* seqs, int* lengths, int* steps_run,
                     int* err_flag, hipStream_t s) {
  return beam_loop(nlayers, n, k, H, V, max_steps, start_token, end_token, Cw, Cb, state0, ws, slab, slab_floats, poll_every, seqs,
                   lengths, steps_run, s,
                   [&](const long long* tok, const long long* parent, const float* sin, float* sout, float* h_top) {
                     const bool given = !parent && first_inputs;     // step 1 on the caller's rows
                     return stacked_decode_step(cell, nlayers, n * k, E, H, V, given ? nullptr : tok, given ? first_inputs : emb,
                                                wcat, beff, sin, sout, h_top, err_flag, s, parent);
                   },
                   fused_topk != 0);
}

// ---- every emotion decoder of capnet.seq2seq in one search: groups x n sentences, group g on its own embedding, LSTM
// weights and projection (the decode step on a (H / 4, groups) grid with per-group tables, parents gathered in the kernel)
size_t lstm_beam_decode_groups_ws_bytes(int nlayers, int groups, int n, int k, int H, int V, int max_steps, int fused_topk) {
  if (groups < 1 || groups > 8 || n < 1 || n >= (1 << 24)) return 0;
  if (!lstm_beam_decode_ws_bytes(nlayers, groups * n, k, H, V, max_steps, fused_topk)) return 0;
  return beam_decode_layout(nlayers, groups * n, k, H, V, max_steps, fused_topk != 0, groups).total;
}

int lstm_beam_decode_groups(int cell, int nlayers, int groups, int n, int k, int E, int H, int V, int max_steps,
                            long long start_token, long long end_token, const float* const* emb, const float* const* wcat,
                            const float* const* beff, const float* const* Cw, const float* const* Cb, const float* state0,
                            void* ws, float* slab, size_t slab_floats, int fused_topk, int poll_every, long long* seqs,
                            int* lengths, int* steps_run, int* err_flag, hipStream_t s) {
  const int nq = groups * n;
  return beam_loop(nlayers, nq, k, H, V, max_steps, start_token, end_token, nullptr, nullptr, state0, ws, slab, slab_floats,
                   poll_every, seqs, lengths, steps_run, s,
                   [&](const long long* tok, const long long* parent, const float* sin, float* sout, float* h_top) {
                     return stacked_decode_step(cell, nlayers, nq * k, E, H, V, tok, emb[0], wcat, beff, sin, sout, h_top, err_flag,
                                                s, parent, groups, emb);
                   },
                   fused_topk != 0, groups, Cw, Cb);
}

// ---- the same loop for the attention decoders: the step is att_decode_step (z, the two attention launches, layer 0 on
// [embedding | gated context], the upper layers) ----
// ws: beam_decode's layout, then att_decode_step's block (z | xa | escore)
// the maps of the winners out of the per-step history: workgroup (i, e) copies hist[e][rows[i][e]] -- the row hypothesis i
// occupied at step e + 1 -- to alphas[i][e]; a row of -1 (past the caption, nothing completed) or out of range gives zeros
__global__ __launch_bounds__(256) void alpha_gather_kernel(const float* __restrict__ hist, const int* __restrict__ rows, int nk,
                                                           int max_steps, int P, float* __restrict__ alphas) {
  const int i = blockIdx.x, e = blockIdx.y;
  const int r = rows[(long)i * max_steps + e];
  const bool ok = r >= 0 && r < nk;
  const float* src = hist + ((size_t)e * nk + (ok ? r : 0)) * P;
  float* dst = alphas + ((size_t)i * max_steps + e) * P;
  for (int p = threadIdx.x; p < P; p += 256) dst[p] = ok ? src[p] : 0.f;
}

size_t att_beam_decode_ws_bytes(int nlayers, int n, int k, int P, int A, int C, int E, int H, int V, int max_steps) {
  const size_t base = beam_decode_ws_bytes(nlayers, n, k, H, V, max_steps), step = att_decode_step_ws_bytes(n, k, P, A, C, E);
  return base && step ? base + gd_align(step) : 0;
}

int att_beam_decode(int cell, int nlayers, int n, int k, int P, int A, int C, int E, int H, int V, int max_steps,
                    long long start_token, long long end_token, const float* att1, const float* feat, const float* emb,
                    const float* wz, const float* bz, const float* wf, const float* bf, const float* const* wcat,
                    const float* const* beff, const float* Cw, const float* Cb, const float* state0, void* ws, float* slab,
                    size_t slab_floats, int poll_every, long long* seqs, int* lengths, int* steps_run, int* err_flag,
                    hipStream_t s, int groups, float* alphas) {
  const int nq = groups * n;   // beam groups: weight groups x images, group-major
  char* p = reinterpret_cast<char*>(ws);
  void* step_ws = p + beam_decode_layout(nlayers, nq, k, H, V, max_steps).total;
  // the maps (alphas set): behind the search's own workspace, trace | rows int32 [nq][max_steps] | history
  // [max_steps][nq k][P] -- step e's attention writes slice e - 1, the advance records the rows, one gather at the end
  void* trace = nullptr;
  int* rows = nullptr;
  float* hist = nullptr;
  if (alphas) {
    p += att_beam_decode_ws_bytes(nlayers, nq, k, P, A, C, E, H, V, max_steps);
    trace = p;
    p += gd_align(beam_trace_bytes(nq, k, max_steps));
    rows = reinterpret_cast<int*>(p);
    p += gd_align((size_t)nq * max_steps * sizeof(int));
    hist = reinterpret_cast<float*>(p);
  }
  int calls = 0;   // the step the loop is at: it calls the step once per step, in order
  const int rc = beam_loop(
      nlayers, nq, k, H, V, max_steps, start_token, end_token, Cw, Cb, state0, ws, slab, slab_floats, poll_every, seqs, lengths,
      steps_run, s,
      [&](const long long* tok, const long long* parent, const float* sin, float* sout, float* h_top) {
        float* slice = hist ? hist + (size_t)calls++ * nq * k * P : nullptr;
        return att_decode_step(cell, nlayers, n, k, P, A, C, E, H, V, att1, feat, tok, emb, wz, bz, wf, bf, wcat, beff, sin, parent,
                               sout, h_top, step_ws, slab, slab_floats, err_flag, s, groups, slice);
      },
      false, 1, nullptr, nullptr, trace, rows);
  if (rc != kOk || !alphas) return rc;
  hipLaunchKernelGGL(alpha_gather_kernel, dim3(nq, max_steps), dim3(256), 0, s, hist, rows, nq * k, max_steps, P, alphas);
  CAPNET_LAUNCH_CHECK();
  return kOk;
}

size_t att_beam_decode_alphas_ws_bytes(int nlayers, int groups, int n, int k, int P, int A, int C, int E, int H, int V,
                                       int max_steps) {
  if (groups < 1 || groups > 8 || n < 1 || n >= (1 << 24)) return 0;
  const int nq = groups * n;
  const size_t base = att_beam_decode_ws_bytes(nlayers, nq, k, P, A, C, E, H, V, max_steps);
  if (!base) return 0;
  return base + gd_align(beam_trace_bytes(nq, k, max_steps)) + gd_align((size_t)nq * max_steps * sizeof(int)) +
         gd_align((size_t)max_steps * nq * k * P * sizeof(float));
}

// ---- what the searches leave in the caller's workspace (capnet_beam_nbest after the search returns) ----
size_t beam_decode_ws_beam_offset(int nlayers, int n, int k, int H, int V, int max_steps, int fused_topk, int groups) {
  if (!lstm_beam_decode_groups_ws_bytes(nlayers, groups, n, k, H, V, max_steps, fused_topk)) return 0;
  return beam_decode_layout(nlayers, groups * n, k, H, V, max_steps, fused_topk != 0, groups).beam;
}

size_t att_beam_decode_alphas_ws_trace_offset(int nlayers, int groups, int n, int k, int P, int A, int C, int E, int H, int V,
                                              int max_steps) {
  if (!att_beam_decode_alphas_ws_bytes(nlayers, groups, n, k, P, A, C, E, H, V, max_steps)) return 0;
  return att_beam_decode_ws_bytes(nlayers, groups * n, k, P, A, C, E, H, V, max_steps);
}

size_t att_beam_decode_alphas_ws_hist_offset(int nlayers, int groups, int n, int k, int P, int A, int C, int E, int H, int V,
                                             int max_steps) {
  const size_t trace = att_beam_decode_alphas_ws_trace_offset(nlayers, groups, n, k, P, A, C, E, H, V, max_steps);
  if (!trace) return 0;
  const int nq = groups * n;
  return trace + gd_align(beam_trace_bytes(nq, k, max_steps)) + gd_align((size_t)nq * max_steps * sizeof(int));
}

int alpha_gather(const float* hist, const int* rows, int captions, int nk, int max_steps, int P, float* alphas, hipStream_t s) {
  CAPNET_REQUIRE(hist && rows && alphas, "alpha_gather: null argument");
  CAPNET_REQUIRE((size_t)hist % 4 == 0 && (size_t)rows % 4 == 0 && (size_t)alphas % 4 == 0,
                 "alpha_gather: hist, rows and alphas must be 4-byte aligned");
  CAPNET_REQUIRE(captions >= 1 && nk >= 1 && max_steps >= 1 && max_steps <= 65535 && P >= 1,
                 "alpha_gather: captions=%d nk=%d max_steps=%d P=%d (all >= 1, max_steps <= 65535)", captions, nk, max_steps, P);
  hipLaunchKernelGGL(alpha_gather_kernel, dim3(captions, max_steps), dim3(256), 0, s, hist, rows, nk, max_steps, P, alphas);
  CAPNET_LAUNCH_CHECK();
  return kOk;
}

}  // namespace capnet
