// A beam step's vocabulary projection without its logits: per row the k best entries and the row's log-sum-exp in ONE
// launch (capnet_vocab_topk), what capnet_beam_advance_topk needs of a step instead of the [rows][V] block.
//   logit[r][v] = h[r] . W[v] + b[v]        h [rows][H], W [V][H] (nn.Linear), b [V]
//   index[r][0..k) the k best v by (logit descending, v ascending), values[r][j] their logits, lse[r] = log sum_v exp(logit)
//
// Mapping: vocab_argmax_kernel's (vocab_argmax.hip). A workgroup owns 32 vocabulary entries = two N tiles of the 16-row
// product (step_core.h) and ALL rows; its 8 waves are 2 tiles x 4 contiguous quarters of K = H; a lane loads its column's
// weights for its quarter once and keeps them while the workgroup walks the rows 16 TM at a time. The four K-partial tiles
// are summed through LDS in a fixed order and the bias is added: a row's 32 logits sit in the 32 lanes of half a wave.
// Per row the workgroup emits
//   m_w = the maximum of its pickable logits, s_w = sum expf(logit - m_w) over them (one packed 8-byte word), and
//   its min(k, 32) best (value, index) words, best first: a lane's rank is the number of lanes that beat it under the
//   total order (value descending, index ascending), read off 32 lane broadcasts; ranks below k store.
// A logit that is NaN or -inf, or lies beyond V, is not pickable: it is ranked behind every pickable one, never stored and
// adds nothing to s_w; the slots a workgroup cannot fill hold (-inf, -1).
// Cross-workgroup: vocab_argmax_kernel's hand-off, cell by cell -- every partial an 8-byte agent-scope store, every storing
// wave drained, a workgroup barrier, one lane's agent-scope atomic add on the one counter, the partials read back with
// agent-scope loads by the workgroup that arrives LAST. No workgroup waits on another. The last one merges, lpr = 64, 32 or
// 16 lanes per row (by the row count alone: up to 8, 16, more), the rows of a pass side by side:
//   M = max m_w, S = sum s_w expf(m_w - M) with lane l adding workgroups l, l + lpr, ... in that order and the lanes then
//   combined by the xor tree, lse = M + logf(S): the same bits whoever arrives last;
//   the k best of the workgroups' candidates. Every workgroup's list is sorted, so a lane keeps the best HEAD of the lists
//   it owns (workgroups l, l + lpr, ...): k rounds of one lpr-lane reduction under the same total order, after which only
//   the winning lane re-reads its lists' heads (a list's head position is the number of winners so far in its 32
//   columns). A row with fewer than k pickable entries pads with (-inf, -1).
// The counter is zero before the first use and zero again when the launch ends. Plain vector loads and stores only.
// Weight groups (every emotion of capnet.seq2seq at once: capnet_vocab_topk_groups, capnet_lstm_beam_decode_groups):
// vocab_argmax_kernel's grouping to the letter. The grid is (ceil(V / 32), G), rows are group-major, and workgroup (., g)
// walks only rows [g rpg, (g + 1) rpg) on w[g] / b[g] -- one pointer per group held by value in the argument struct and picked
// by blockIdx.y, a scalar load from the kernel arguments; no projection is stacked or copied. Everything below the pick
// works on the group's own rows, numbered from 0: the row clamp and the store mask end at the group, so a 16-row tile
// never reaches into the next one. Group g owns its block of stat and cand and its OWN arrival counter (16 bytes apart),
// where arrivals are counted against gridDim.x: group g's last arriver merges group g's rows only (lpr by rpg, not by the
// total row count) and re-arms that counter only. The groups never meet. G = 1 is the kernel as it was: the same grid,
// the same addresses, the same bits.
#include "common.h"
#include "kernels.h"
#include "step_core.h"

namespace capnet {

constexpr int kVtWaves = 8;
constexpr int kVtCols = 32;          // vocabulary entries per workgroup
constexpr int kVtNone = 0x7fffffff;
constexpr int kVtMaxK = 16;
constexpr int kVtBatch = 8;          // independent loads in flight per lane in the merge

constexpr int kVtMaxGroups = 8;      // weight groups of one launch

struct VocabTopkArgs {
  const float* h;            // [groups rpg][H], group-major
  unsigned long long* stat;  // [groups][workgroups][rpg]: (m_w bits << 32) | s_w bits
  unsigned long long* cand;  // [groups][workgroups][rpg][k]: (value bits << 32) | index, best first; index -1 = nothing
  int* counter;              // group g's at counter + 4 g; zero before the first use, zero again when the launch ends
  float* values;             // [groups rpg][k]
  int* index;                // [groups rpg][k]
  float* lse;                // [groups rpg]
  int rpg, H, V, k;          // rows per group: workgroup (., g) owns rows [g rpg, (g + 1) rpg)
  const float* w[kVtMaxGroups];   // [V][H] of group g
  const float* b[kVtMaxGroups];   // [V] of group g, or null
};

__device__ __forceinline__ unsigned long long vt_pack(float hi, unsigned lo) {
  return ((unsigned long long)__float_as_uint(hi) << 32) | lo;
}
__device__ __forceinline__ void vt_store(unsigned long long* p, unsigned long long u) {
  __hip_atomic_store(p, u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long vt_load(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ bool vt_better(float v, int i, float best, int bi) {
  return v > best || (v == best && i < bi);
}

template <int NJ, int TM>
__global__ __launch_bounds__(512) void vocab_topk_kernel(VocabTopkArgs a) {
  constexpr int kPass = 16 * TM;
  __shared__ float red[kVtWaves][kPass][17];
  __shared__ int s_last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lq = lane >> 4;
  const int tile = wave >> 2, ks = wave & 3;
  const int H = a.H, rows = a.rpg, k = a.k, c0 = blockIdx.x * kVtCols;
  // this group's rows, numbered from 0 below: its slice of h and of the outputs, its blocks of stat and cand, its counter
  const int grp = blockIdx.y;
  const long rbeg = (long)grp * rows;
  const float* gh = a.h + rbeg * H;
  const float* bg = a.b[grp];
  unsigned long long* gstat = a.stat + (long)grp * gridDim.x * rows;
  unsigned long long* gcand = a.cand + (long)grp * gridDim.x * rows * k;
  float* gvalues = a.values + rbeg * k;
  int* gindex = a.index + rbeg * k;
  float* glse = a.lse + rbeg;
  int* gcounter = a.counter + 4 * grp;
  const int g0 = ks * NJ;                                   // this wave's k groups [g0, g0 + NJ): H = 64 NJ
  const int wcol = clamp_row(c0 + 16 * tile + li, a.V);      // entries beyond V: masked in the epilogue
  const float* wrow = a.w[grp] + (long)wcol * H + 16 * g0 + 4 * lq;
  f32x4 wv[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) wv[j] = *reinterpret_cast<const f32x4*>(wrow + 16 * j);
  // epilogue thread: (row er of a 16-row tile, entry ec of the workgroup's 32)
  const int er = tid >> 5, ec = tid & 31;
  const int ecol = c0 + ec;
  const float bias = (bg && ecol < a.V) ? bg[ecol] : 0.f;
  unsigned long long* stat = gstat + (long)blockIdx.x * rows;
  unsigned long long* cand = gcand + (long)blockIdx.x * rows * k;
  for (int r0 = 0; r0 < rows; r0 += kPass) {
    f32x4 acc[TM];
#pragma unroll
    for (int m = 0; m < TM; ++m) {
      const int row = clamp_row(r0 + 16 * m + li, rows);
      const float* hrow = gh + (long)row * H + 16 * g0 + 4 * lq;
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
      const bool ok = ecol < a.V && v > -INFINITY;          // NaN fails the comparison
      const float pv = ok ? v : -INFINITY;
      float mx = pv;                                        // the row's 32 threads are one half of a wave
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
      float e = ok ? expf(pv - mx) : 0.f;
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) e += __shfl_xor(e, o);
      int rank = 0;
#pragma unroll
      for (int j = 0; j < 32; ++j) {
        const float ov = __shfl(pv, j, 32);
        rank += (ov > pv || (ov == pv && j < ec)) ? 1 : 0;
      }
      const unsigned long long bal = __ballot(ok);
      const int cnt = __popcll(lane < 32 ? (bal & 0xffffffffULL) : (bal >> 32));   // pickable entries: ranks 0 .. cnt - 1
      if (row < rows) {
        unsigned long long* c = cand + (long)row * k;
        if (ok && rank < k) vt_store(c + rank, vt_pack(v, (unsigned)ecol));
        if (ec >= cnt && ec < k) vt_store(c + ec, vt_pack(-INFINITY, 0xffffffffu));
        if (ec == 0) vt_store(stat + row, vt_pack(mx, __float_as_uint(e)));
      }
    }
    __syncthreads();   // red is rewritten by the next pass
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0)
    s_last = __hip_atomic_fetch_add(gcounter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1;
  __syncthreads();
  if (!s_last) return;
  // the group's last arriver: `lpr` lanes per row (a whole wave for few rows, a quarter for many: the merge of a row is a chain of
  // dependent loads, so rows side by side hide it), the workgroups across those lanes. Every lane runs every shuffle; a
  // lane group without a row works on a copy of the last row and stores nothing.
  const int nwg = gridDim.x;
  const int lpr = rows <= kVtWaves ? 64 : rows <= 2 * kVtWaves ? 32 : 16;
  const int rpw = 64 / lpr, sub = lane / lpr, sl = lane & (lpr - 1);
  for (int base = 0; base < rows; base += kVtWaves * rpw) {
    const int rr = base + wave * rpw + sub;
    const bool valid = rr < rows;
    const int row = valid ? rr : rows - 1;
    // lse: M, then S in a fixed order
    // (every loop over a lane's workgroups issues kVtBatch independent loads before it uses one: the loads are L2 round
    // trips, and one after the other they were the whole cost of the merge)
    float M = -INFINITY;
    for (int p0 = sl; p0 < nwg; p0 += kVtBatch * lpr) {
      unsigned long long u[kVtBatch];
#pragma unroll
      for (int q = 0; q < kVtBatch; ++q) u[q] = vt_load(gstat + (long)min(p0 + q * lpr, nwg - 1) * rows + row);
#pragma unroll
      for (int q = 0; q < kVtBatch; ++q)
        if (p0 + q * lpr < nwg) M = fmaxf(M, __uint_as_float((unsigned)(u[q] >> 32)));
    }
    for (int o = lpr >> 1; o > 0; o >>= 1) M = fmaxf(M, __shfl_xor(M, o));
    float S = 0.f;
    for (int p0 = sl; p0 < nwg; p0 += kVtBatch * lpr) {
      unsigned long long u[kVtBatch];
#pragma unroll
      for (int q = 0; q < kVtBatch; ++q) u[q] = vt_load(gstat + (long)min(p0 + q * lpr, nwg - 1) * rows + row);
#pragma unroll
      for (int q = 0; q < kVtBatch; ++q) {
        const float mw = __uint_as_float((unsigned)(u[q] >> 32)), sw = __uint_as_float((unsigned)u[q]);
        if (p0 + q * lpr < nwg && mw > -INFINITY) S += sw * expf(mw - M);
      }
    }
    for (int o = lpr >> 1; o > 0; o >>= 1) S += __shfl_xor(S, o);
    if (sl == 0 && valid) glse[row] = M + logf(S);
    // the k best: `sel` holds the winners so far (every lane of the row the same)
    int sel[kVtMaxK];
#pragma unroll
    for (int q = 0; q < kVtMaxK; ++q) sel[q] = -1;
    float hv = -INFINITY;    // the best head of this lane's lists
    int hi = kVtNone;
    bool rescan = true;
    for (int j = 0; j < k; ++j) {
      if (rescan) {
        hv = -INFINITY;
        hi = kVtNone;
        for (int p0 = sl; p0 < nwg; p0 += kVtBatch * lpr) {
          unsigned long long u[kVtBatch];
          bool live[kVtBatch];
#pragma unroll
          for (int b = 0; b < kVtBatch; ++b) {
            const int p = min(p0 + b * lpr, nwg - 1);
            int pos = 0;
#pragma unroll
            for (int q = 0; q < kVtMaxK; ++q) pos += (sel[q] >= 0 && (sel[q] >> 5) == p) ? 1 : 0;
            live[b] = p0 + b * lpr < nwg && pos < k;
            u[b] = vt_load(gcand + ((long)p * rows + row) * k + min(pos, k - 1));
          }
#pragma unroll
          for (int b = 0; b < kVtBatch; ++b) {
            const float v = __uint_as_float((unsigned)(u[b] >> 32));
            const int i = (int)(unsigned)u[b];
            if (live[b] && i >= 0 && vt_better(v, i, hv, hi)) { hv = v; hi = i; }
          }
        }
      }
      float bv = hv;
      int bi = hi;
      for (int o = lpr >> 1; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        if (vt_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
      }
      const bool none = bi == kVtNone;       // (the same in every lane of the row) nothing left: this slot and the rest are padding
      if (sl == 0 && valid) {
        gvalues[(long)row * k + j] = none ? -INFINITY : bv;
        gindex[(long)row * k + j] = none ? -1 : bi;
      }
#pragma unroll
      for (int q = 0; q < kVtMaxK; ++q)
        if (q == j) sel[q] = none ? -1 : bi;
      rescan = !none && ((bi >> 5) & (lpr - 1)) == sl;
    }
  }
  if (tid == 0) __hip_atomic_store(gcounter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

static int vt_workgroups(int V) { return (V + kVtCols - 1) / kVtCols; }

bool vocab_topk_supported(int H, int k, int V) { return step_hidden_supported(H) && k >= 1 && k <= kVtMaxK && k <= V; }

// workspace: per group 16 bytes whose first int is the group's counter | stat [groups][workgroups][rpg] | cand
// [groups][workgroups][rpg][k], 8-byte words
size_t vocab_topk_groups_ws_bytes(int groups, int rpg, int k, int V) {
  if (groups < 1 || groups > kVtMaxGroups || rpg < 1 || k < 1 || k > kVtMaxK || V < k) return 0;
  return 16 * (size_t)groups + (size_t)groups * vt_workgroups(V) * rpg * 8 * (1 + (size_t)k);
}
size_t vocab_topk_ws_bytes(int rows, int k, int V) { return vocab_topk_groups_ws_bytes(1, rows, k, V); }

int vocab_topk(const float* h, const float* w, const float* b, int rows, int H, int V, int k, void* ws, float* values,
               int* index, float* lse, hipStream_t stream) {
  return vocab_topk_groups(h, &w, b ? &b : nullptr, 1, rows, H, V, k, ws, values, index, lse, stream);
}

int vocab_topk_groups(const float* h, const float* const* w, const float* const* b, int groups, int rpg, int H, int V, int k,
                      void* ws, float* values, int* index, float* lse, hipStream_t stream) {
  CAPNET_REQUIRE(groups >= 1 && groups <= kVtMaxGroups && rpg >= 1 && vocab_topk_supported(H, k, V),
                 "vocab_topk: %d groups of %d rows, H %d, V %d, k %d", groups, rpg, H, V, k);
  VocabTopkArgs a;
  a.h = h;
  for (int g = 0; g < kVtMaxGroups; ++g) {
    a.w[g] = w[g < groups ? g : 0];
    a.b[g] = b ? b[g < groups ? g : 0] : nullptr;
  }
  a.counter = reinterpret_cast<int*>(ws);
  a.stat = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(ws) + 16 * (size_t)groups);
  a.cand = a.stat + (size_t)groups * vt_workgroups(V) * rpg;
  a.values = values; a.index = index; a.lse = lse;
  a.rpg = rpg; a.H = H; a.V = V; a.k = k;
  const dim3 grid(vt_workgroups(V), groups), block(64 * kVtWaves);
  dispatch_nj(H, [&](auto nj) {   // two row tiles per pass where their operands fit beside the weights
    hipLaunchKernelGGL((vocab_topk_kernel<nj, nj <= 8 ? 2 : 1>), grid, block, 0, stream, a);
  });
  CAPNET_LAUNCH_CHECK();
  return kOk;
}

}  // namespace capnet
