// What the vocabulary kernels share (vocab_argmax.hip, vocab_topk.hip, vocab_sample.hip): the projection front, the
// cross-workgroup hand-off, the half-wave (m_w, s_w) reduction, the packed words and the per-group argument block.
//   logit[r][v] = h[r] . W[v] + b[v]        h [rows][H], W [V][H] (nn.Linear), b [V]
// Mapping (the arrangement of lstm_decode_step.hip): a workgroup owns 32 vocabulary entries = two N tiles of the 16-row
// product (step_core.h) and ALL rows of its group. Its 8 waves are 2 tiles x 4 contiguous quarters of K = H; a lane loads
// its column's weights for its quarter once (NJ f32x4 registers: the projection crosses the memory system once per launch)
// and keeps them while the workgroup walks the rows 16 TM at a time. The four K-partial tiles are summed through LDS in a
// fixed order and the bias is added: a row's 32 logits sit in the 32 lanes of half a wave, where the kernel's epilogue
// reduces them and stores the workgroup's partials of the row. Plain vector loads and stores only.
// Weight groups: the grid is (ceil(V / 32), G), rows are group-major, and workgroup (., g) walks only rows [g rpg, (g + 1)
// rpg) on w[g] / b[g] -- one pointer per group held by value in the argument struct (VocabGroups) and picked by blockIdx.y,
// a scalar load from the kernel arguments; no projection is stacked or copied. The front sees a group's rows numbered from
// 0: the row clamp and the store mask end at the group, so a 16-row tile never reaches into the next one. Group g owns its
// blocks of partials and its OWN arrival counter (16 bytes apart), where arrivals are counted against gridDim.x; the groups
// never meet. G = 1 is the one-group kernel: the same grid, the same addresses, the same bits.
#pragma once
#include "step_core.h"

namespace capnet {

constexpr int kVocWaves = 8;
constexpr int kVocCols = 32;          // vocabulary entries per workgroup
constexpr int kVocNone = 0x7fffffff;  // the index of "nothing to pick"
constexpr int kVocMaxGroups = 8;      // weight groups of one launch

static inline int vocab_workgroups(int V) { return (V + kVocCols - 1) / kVocCols; }

struct VocabGroups {
  const float* w[kVocMaxGroups];   // [V][H] of group g
  const float* b[kVocMaxGroups];   // [V] of group g, or null
};
// host-side tables w / b of `groups` pointers (b or any b[g] may be null); the slots past the last group repeat group 0
static inline void vocab_fill_groups(VocabGroups& t, const float* const* w, const float* const* b, int groups) {
  for (int g = 0; g < kVocMaxGroups; ++g) {
    t.w[g] = w[g < groups ? g : 0];
    t.b[g] = b ? b[g < groups ? g : 0] : nullptr;
  }
}

// the total order of the reductions: value descending, index ascending. NaN never wins; the winner of a set does not
// depend on the order in which its members meet
__device__ __forceinline__ bool vocab_better(float v, int i, float best, int bi) {
  return v > best || (v == best && i < bi);
}
// a partial: two 32-bit halves in one 8-byte word, (value, index) or (m_w, s_w)
__device__ __forceinline__ unsigned long long vocab_pack(float hi, unsigned lo) {
  return ((unsigned long long)__float_as_uint(hi) << 32) | lo;
}
__device__ __forceinline__ float vocab_hi(unsigned long long u) { return __uint_as_float((unsigned)(u >> 32)); }
__device__ __forceinline__ unsigned vocab_lo(unsigned long long u) { return (unsigned)u; }
template <class T>
__device__ __forceinline__ void vocab_store(T* p, T u) {
  __hip_atomic_store(p, u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <class T>
__device__ __forceinline__ T vocab_load(const T* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The front: rows [0, rows) at h on w / b (a group's, already resolved). Every thread calls epi(row, valid, logit) once per
// row tile of every pass, as thread (row er of the tile, entry ec = threadIdx.x & 31 of the workgroup's 32): logit is
// that of (row, entry blockIdx.x 32 + ec), valid says the row exists. The epilogues shuffle across the row's 32 lanes, so
// the call is unconditional; an entry beyond V is a clamped copy with bias 0 that the epilogue masks. Only additions and
// the MFMA builtin here: nothing a contraction mode could change.
template <int NJ, int TM, class Epi>
__device__ __forceinline__ void vocab_front(const float* h, int rows, const float* w, const float* b, int H, int V, Epi&& epi) {
  constexpr int kPass = 16 * TM;
  __shared__ float red[kVocWaves][kPass][17];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lq = lane >> 4;
  const int tile = wave >> 2, ks = wave & 3;
  const int c0 = blockIdx.x * kVocCols;
  const int g0 = ks * NJ;                                   // this wave's k groups [g0, g0 + NJ): H = 64 NJ
  const int wcol = clamp_row(c0 + 16 * tile + li, V);        // entries beyond V: masked in the epilogue
  const float* wrow = w + (long)wcol * H + 16 * g0 + 4 * lq;
  f32x4 wv[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) wv[j] = *reinterpret_cast<const f32x4*>(wrow + 16 * j);
  const int er = tid >> 5, ec = tid & 31;
  const int ecol = c0 + ec;
  const float bias = (b && ecol < V) ? b[ecol] : 0.f;
  for (int r0 = 0; r0 < rows; r0 += kPass) {
    f32x4 acc[TM];
#pragma unroll
    for (int m = 0; m < TM; ++m) {
      const int row = clamp_row(r0 + 16 * m + li, rows);
      const float* hrow = h + (long)row * H + 16 * g0 + 4 * lq;
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
      epi(row, row < rows, bias + red[t4][pr][cc] + red[t4 + 1][pr][cc] + red[t4 + 2][pr][cc] + red[t4 + 3][pr][cc]);
    }
    __syncthreads();   // red is rewritten by the next pass
  }
}

// The row's (m_w, s_w) over its 32 lanes, one half of a wave: pv is the lane's logit where it is pickable (ok), else -inf;
// mx = the maximum, e = sum expf(pv - mx) over the pickable lanes. The same value in all 32 lanes.
__device__ __forceinline__ void vocab_half_wave_stat(bool ok, float pv, float& mx, float& e) {
  mx = pv;
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  e = ok ? expf(pv - mx) : 0.f;
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) e += __shfl_xor(e, o);
}

// The hand-off (gemm_rows16_kernel's in gemm_f32.hip, cell by cell). A workgroup writes its partials with agent-scope
// stores (vocab_store) and then calls arrive_last, all threads: every storing wave drains its stores, a workgroup barrier,
// ONE lane's relaxed agent-scope atomic add on the group's counter, a barrier again. The workgroup that finds the counter
// at `workgroups` - 1 arrived LAST: it gets true, reads every workgroup's partials back with agent-scope loads (vocab_load)
// and merges them; the others return. No workgroup waits on another. What the last arriver computes must not depend on who
// it is: the reductions are total orders or sums in a fixed order. It ends with vocab_rearm: the counter is zero before the
// first use and zero again when the launch ends.
__device__ __forceinline__ bool arrive_last(int* counter, int workgroups) {
  __shared__ int s_last;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0)
    s_last = __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == workgroups - 1;
  __syncthreads();
  return s_last;
}
__device__ __forceinline__ void vocab_rearm(int* counter) {
  if (threadIdx.x == 0) vocab_store(counter, 0);
}

}  // namespace capnet
