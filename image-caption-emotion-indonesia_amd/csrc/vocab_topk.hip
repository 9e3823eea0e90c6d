// A beam step's vocabulary projection without its logits: per row the k best entries and the row's log-sum-exp in ONE
// launch (capnet_vocab_topk), what capnet_beam_advance_topk needs of a step instead of the [rows][V] block.
//   logit[r][v] = h[r] . W[v] + b[v]        h [rows][H], W [V][H] (nn.Linear), b [V]
//   index[r][0..k) the k best v by (logit descending, v ascending), values[r][j] their logits, lse[r] = log sum_v exp(logit)
//
// The mapping, the weight groups and the hand-off are vocab_core.h's. Per row the workgroup emits
//   m_w = the maximum of its pickable logits, s_w = sum expf(logit - m_w) over them (one packed 8-byte word), and
//   its min(k, 32) best (value, index) words, best first: a lane's rank is the number of lanes that beat it under the
//   total order (value descending, index ascending), read off 32 lane broadcasts; ranks below k store.
// A logit that is NaN or -inf, or lies beyond V, is not pickable: it is ranked behind every pickable one, never stored and
// adds nothing to s_w; the slots a workgroup cannot fill hold (-inf, -1).
// The group's last arriver merges, lpr = 64, 32 or 16 lanes per row (by the group's row count alone: up to 8, 16, more),
// the rows of a pass side by side:
//   M = max m_w, S = sum s_w expf(m_w - M) with lane l adding workgroups l, l + lpr, ... in that order and the lanes then
//   combined by the xor tree, lse = M + logf(S): the same bits whoever arrives last (the sum contracts into fused
//   multiply-adds here and does not in vocab_sample.hip: each kernel keeps its own merge and its own rounding);
//   the k best of the workgroups' candidates. Every workgroup's list is sorted, so a lane keeps the best HEAD of the lists
//   it owns (workgroups l, l + lpr, ...): k rounds of one lpr-lane reduction under the same total order, after which only
//   the winning lane re-reads its lists' heads (a list's head position is the number of winners so far in its 32
//   columns). A row with fewer than k pickable entries pads with (-inf, -1).
#include "common.h"
#include "kernels.h"
#include "vocab_core.h"

namespace capnet {

constexpr int kVtMaxK = 16;
constexpr int kVtBatch = 8;          // independent loads in flight per lane in the merge

struct VocabTopkArgs {
  const float* h;            // [groups rpg][H], group-major
  unsigned long long* stat;  // [groups][workgroups][rpg]: (m_w bits << 32) | s_w bits
  unsigned long long* cand;  // [groups][workgroups][rpg][k]: (value bits << 32) | index, best first; index -1 = nothing
  int* counter;              // group g's at counter + 4 g; zero before the first use, zero again when the launch ends
  float* values;             // [groups rpg][k]
  int* index;                // [groups rpg][k]
  float* lse;                // [groups rpg]
  int rpg, H, V, k;          // rows per group: workgroup (., g) owns rows [g rpg, (g + 1) rpg)
  VocabGroups g;
  const unsigned* mask;      // masked instances only: [groups rpg][workgroups], bit c of word b = entry 32 b + c of that row
};

// The three instances by what a set mask bit means (one 4-byte load per half-wave; the unmasked kernel reads no mask):
//   kVtPickMask (the sampler's, sample_exclude.hip): the entry is treated as a -inf logit is, so the k best AND lse
//     are those of the allowed entries -- the distribution renormalised over them;
//   kVtSelectMask (the constrained beam search's): the entry only leaves the SELECTION -- it is not ranked, not
//     counted and never stored as a candidate, but (m_w, s_w) is formed from every finite in-range logit exactly as in the
//     unmasked instance, so lse is the unmasked launch's bit for bit and a survivor's score stays the model's own
//     log-probability.
constexpr int kVtNoMask = 0, kVtPickMask = 1, kVtSelectMask = 2;
template <int NJ, int TM, int MASK>
__global__ __launch_bounds__(512) void vocab_topk_kernel(VocabTopkArgs a) {
  const int rows = a.rpg, k = a.k;
  // this group's rows, numbered from 0 below: its slice of h and of the outputs, its blocks of stat and cand, its counter
  const int grp = blockIdx.y;
  const long rbeg = (long)grp * rows;
  unsigned long long* gstat = a.stat + (long)grp * gridDim.x * rows;
  unsigned long long* gcand = a.cand + (long)grp * gridDim.x * rows * k;
  float* gvalues = a.values + rbeg * k;
  int* gindex = a.index + rbeg * k;
  float* glse = a.lse + rbeg;
  int* gcounter = a.counter + 4 * grp;
  unsigned long long* stat = gstat + (long)blockIdx.x * rows;
  unsigned long long* cand = gcand + (long)blockIdx.x * rows * k;
  vocab_front<NJ, TM>(a.h + rbeg * a.H, rows, a.g.w[grp], a.g.b[grp], a.H, a.V, [&](int row, bool valid, float v) {
    const int lane = threadIdx.x & 63, ec = lane & 31, ecol = blockIdx.x * kVocCols + ec;   // the thread's entry
    const bool fin = ecol < a.V && v > -INFINITY;         // NaN fails the comparison
    bool ok = fin;                                        // `fin` feeds the statistic, `ok` the rank, the count and the stores
    if (MASK != kVtNoMask) ok = ok && !(valid && ((a.mask[(rbeg + row) * gridDim.x + blockIdx.x] >> ec) & 1u));
    const float pv = ok ? v : -INFINITY;
    float mx, e;
    if (MASK == kVtSelectMask) vocab_half_wave_stat(fin, fin ? v : -INFINITY, mx, e);
    else vocab_half_wave_stat(ok, pv, mx, e);
    int rank = 0;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      const float ov = __shfl(pv, j, 32);
      rank += (ov > pv || (ov == pv && j < ec)) ? 1 : 0;
    }
    const unsigned long long bal = __ballot(ok);
    const int cnt = __popcll(lane < 32 ? (bal & 0xffffffffULL) : (bal >> 32));   // pickable entries: ranks 0 .. cnt - 1
    if (valid) {
      unsigned long long* c = cand + (long)row * k;
      if (ok && rank < k) vocab_store(c + rank, vocab_pack(v, (unsigned)ecol));
      if (ec >= cnt && ec < k) vocab_store(c + ec, vocab_pack(-INFINITY, 0xffffffffu));
      if (ec == 0) vocab_store(stat + row, vocab_pack(mx, __float_as_uint(e)));
    }
  });
  if (!arrive_last(gcounter, gridDim.x)) return;
  // the group's last arriver: `lpr` lanes per row (a whole wave for few rows, a quarter for many: the merge of a row is a chain of
  // dependent loads, so rows side by side hide it), the workgroups across those lanes. Every lane runs every shuffle; a
  // lane group without a row works on a copy of the last row and stores nothing.
  const int nwg = gridDim.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lpr = rows <= kVocWaves ? 64 : rows <= 2 * kVocWaves ? 32 : 16;
  const int rpw = 64 / lpr, sub = lane / lpr, sl = lane & (lpr - 1);
  for (int base = 0; base < rows; base += kVocWaves * rpw) {
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
      for (int q = 0; q < kVtBatch; ++q) u[q] = vocab_load(gstat + (long)min(p0 + q * lpr, nwg - 1) * rows + row);
#pragma unroll
      for (int q = 0; q < kVtBatch; ++q)
        if (p0 + q * lpr < nwg) M = fmaxf(M, vocab_hi(u[q]));
    }
    for (int o = lpr >> 1; o > 0; o >>= 1) M = fmaxf(M, __shfl_xor(M, o));
    float S = 0.f;
    for (int p0 = sl; p0 < nwg; p0 += kVtBatch * lpr) {
      unsigned long long u[kVtBatch];
#pragma unroll
      for (int q = 0; q < kVtBatch; ++q) u[q] = vocab_load(gstat + (long)min(p0 + q * lpr, nwg - 1) * rows + row);
#pragma unroll
      for (int q = 0; q < kVtBatch; ++q) {
        const float mw = vocab_hi(u[q]), sw = __uint_as_float(vocab_lo(u[q]));
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
    int hi = kVocNone;
    bool rescan = true;
    for (int j = 0; j < k; ++j) {
      if (rescan) {
        hv = -INFINITY;
        hi = kVocNone;
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
            u[b] = vocab_load(gcand + ((long)p * rows + row) * k + min(pos, k - 1));
          }
#pragma unroll
          for (int b = 0; b < kVtBatch; ++b) {
            const float v = vocab_hi(u[b]);
            const int i = (int)vocab_lo(u[b]);
            if (live[b] && i >= 0 && vocab_better(v, i, hv, hi)) { hv = v; hi = i; }
          }
        }
      }
      float bv = hv;
      int bi = hi;
      for (int o = lpr >> 1; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        if (vocab_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
      }
      const bool none = bi == kVocNone;       // (the same in every lane of the row) nothing left: this slot and the rest are padding
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
  vocab_rearm(gcounter);
}

bool vocab_topk_supported(int H, int k, int V) { return step_hidden_supported(H) && k >= 1 && k <= kVtMaxK && k <= V; }

// workspace: per group 16 bytes whose first int is the group's counter | stat [groups][workgroups][rpg] | cand
// [groups][workgroups][rpg][k], 8-byte words
size_t vocab_topk_groups_ws_bytes(int groups, int rpg, int k, int V) {
  if (groups < 1 || groups > kVocMaxGroups || rpg < 1 || k < 1 || k > kVtMaxK || V < k) return 0;
  return 16 * (size_t)groups + (size_t)groups * vocab_workgroups(V) * rpg * 8 * (1 + (size_t)k);
}
size_t vocab_topk_ws_bytes(int rows, int k, int V) { return vocab_topk_groups_ws_bytes(1, rows, k, V); }

int vocab_topk(const float* h, const float* w, const float* b, int rows, int H, int V, int k, void* ws, float* values,
               int* index, float* lse, hipStream_t stream, const unsigned* mask, bool select_only) {
  return vocab_topk_groups(h, &w, b ? &b : nullptr, 1, rows, H, V, k, ws, values, index, lse, stream, mask, select_only);
}

int vocab_topk_groups(const float* h, const float* const* w, const float* const* b, int groups, int rpg, int H, int V, int k,
                      void* ws, float* values, int* index, float* lse, hipStream_t stream, const unsigned* mask,
                      bool select_only) {
  CAPNET_REQUIRE(groups >= 1 && groups <= kVocMaxGroups && rpg >= 1 && vocab_topk_supported(H, k, V),
                 "vocab_topk: %d groups of %d rows, H %d, V %d, k %d", groups, rpg, H, V, k);
  VocabTopkArgs a;
  a.h = h;
  vocab_fill_groups(a.g, w, b, groups);
  a.counter = reinterpret_cast<int*>(ws);
  a.stat = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(ws) + 16 * (size_t)groups);
  a.cand = a.stat + (size_t)groups * vocab_workgroups(V) * rpg;
  a.values = values; a.index = index; a.lse = lse;
  a.rpg = rpg; a.H = H; a.V = V; a.k = k;
  a.mask = mask;
  const dim3 grid(vocab_workgroups(V), groups), block(64 * kVocWaves);
  dispatch_nj(H, [&](auto nj) {   // two row tiles per pass where their operands fit beside the weights
    if (mask && select_only) hipLaunchKernelGGL((vocab_topk_kernel<nj, nj <= 8 ? 2 : 1, kVtSelectMask>), grid, block, 0, stream, a);
    else if (mask) hipLaunchKernelGGL((vocab_topk_kernel<nj, nj <= 8 ? 2 : 1, kVtPickMask>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((vocab_topk_kernel<nj, nj <= 8 ? 2 : 1, kVtNoMask>), grid, block, 0, stream, a);
  });
  CAPNET_LAUNCH_CHECK();
  return kOk;
}

}  // namespace capnet
