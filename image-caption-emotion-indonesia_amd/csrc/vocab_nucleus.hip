// Nucleus (top-p) sampling: the draw of sampled decoding among the smallest set of best entries whose probability reaches
// top_p (capnet_nucleus_rows, capnet_nucleus_pick; the sampling loops around them: decode_loops.hip).
//   s_v = z_v inv_T (vs_scaled),  pickable: s_v > -inf (NaN fails) and v < V,  M = max s,  e_v = expf(s_v - M)
//   the total order of vocab_better: s descending, then v ascending
//   before(v) = sum of e_u over the pickable u strictly better than v,  S = sum of e_u over all of them
//   N = { v : before(v) < top_p S }  (top_p S one rounded product): always holds the best entry
//   tok = argmax over N of vs_row_key(s_v, seed, step, row0 + r, greedy_stride, v)  (a greedy row: the best entry, always in N),  logp = s_tok - (M + logf(sum of e_v over N))
// A row with nothing pickable yields token 0 and logp = -inf.
//
// nucleus_rows_kernel: one workgroup per row of a [rows][ld] block of logits. Every sum of the kernel -- S, before(.) at a
// candidate threshold, the kept mass -- is the SAME tree over the same entries with the entries outside the set replaced by
// zero: thread t adds its entries t, t + 256, ... in that order, a wave's 64 partials meet in the xor tree, the four waves'
// sums are added in wave order. Rounding is monotone, so a sum over a subset never exceeds the sum over a superset: before(.)
// as the kernel computes it is non-decreasing along the total order, the set N is a prefix of that order, and its edge is
// found by SEARCH rather than by a sort or a prefix sum:
//   the entries are mapped to 56-bit integers c(v) = (key(s_v) << 24) | (2^24 - 1 - v), key(.) the monotone integer image
//   of a float, so the total order is the integers' descending order;
//   phase 1 finds the smallest K in [key(min s), key(M)] with sum{e_v : key(s_v) > K} < top_p S, 16 ways per pass: each
//   thread evaluates 15 candidate thresholds on its entries in one sweep, the 15 sums are reduced as above, the interval
//   shrinks to the sixteenth between the last failing and the first passing candidate;
//   phase 2, only where more than one entry has key K (equal logits at the edge), finds the smallest c in the tie group's
//   range with sum{e_v : c(v) > c} < top_p S the same way: the index decides.
// N = { v : c(v) >= that c }. No atomics, no dependence on arrival order: one workgroup, barriers and fixed trees. The row's
// scaled logits stay in LDS up to kNucLdsEntries (48 KiB, three workgroups per CU); a longer row is re-read from memory and
// re-scaled in every sweep (the same bits). Any V up to 2^24.
//
// nucleus_pick_kernel: the same rule among the k <= 16 candidates of vocab_topk's (values, index), one thread per row. The
// candidates are walked in the total order (each step picks the best one worse than the last: k^2 reads of at most 16 cached
// values), so neither the set nor the sums depend on the order of the list; S, before and logp are renormalised over the k.
#include "common.h"
#include "kernels.h"
#include "vocab_core.h"
#include "sample_key.h"   // vs_scaled, vs_key; no FMA contraction in this file

namespace capnet {

constexpr int kNucThreads = 256;
constexpr int kNucWaves = kNucThreads / 64;
constexpr int kNucCand = 15;               // candidate thresholds per pass: the interval shrinks 16-fold
constexpr int kNucLdsEntries = 12288;      // scaled logits held in LDS (48 KiB)

// the monotone integer image of a scaled logit (-0 and +0, equal as floats, share one)
__device__ __forceinline__ unsigned nuc_key(float s) {
  const unsigned u = s == 0.f ? 0u : __float_as_uint(s);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ unsigned long long nuc_ckey(float s, int v) {
  return ((unsigned long long)nuc_key(s) << 24) | (unsigned)(0xffffff - v);
}
// a logit as the kernels see it: scaled, and -inf where it is not pickable
__device__ __forceinline__ float nuc_scaled(float z, float inv_T) {
  const float s = vs_scaled(z, inv_T);
  return s > -INFINITY ? s : -INFINITY;
}

// the workgroup's sums of a[0..N): the xor tree over a wave, then the waves in order; every thread gets the totals
template <int N>
__device__ __forceinline__ void nuc_sum(float (&a)[N], float (*part)[kNucWaves]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < N; ++j) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a[j] += __shfl_xor(a[j], o);
    if (lane == 0) part[j][wave] = a[j];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < N; ++j) {
    float t = part[j][0];
#pragma unroll
    for (int w = 1; w < kNucWaves; ++w) t += part[j][w];
    a[j] = t;
  }
  __syncthreads();   // part is rewritten by the next call
}

__global__ __launch_bounds__(kNucThreads) void nucleus_rows_kernel(const float* __restrict__ logits, long ld_logits, int V,
                                                                   float inv_T, float top_p, unsigned long long seed,
                                                                   unsigned step, unsigned row0, unsigned greedy_stride,
                                                                   long long* __restrict__ tok, long long* __restrict__ ids,
                                                                   float* __restrict__ logp, long ld) {
  extern __shared__ float cache[];                     // the row's scaled logits where V <= kNucLdsEntries
  __shared__ float part[kNucCand][kNucWaves];
  __shared__ float pk[kNucWaves], ps[kNucWaves];
  __shared__ int pi[kNucWaves];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* x = logits + (long)row * ld_logits;
  const bool resident = V <= kNucLdsEntries;
  // thread t only ever touches entries t, t + 256, ...: the cache needs no barrier
  auto at = [&](int v) { return resident ? cache[v] : nuc_scaled(x[v], inv_T); };

  // M and the smallest pickable s (the ends of the search), the count of pickable entries
  float M = -INFINITY, lowest = INFINITY;
  for (int v = tid; v < V; v += kNucThreads) {
    const float s = nuc_scaled(x[v], inv_T);
    if (resident) cache[v] = s;
    M = fmaxf(M, s);
    if (s > -INFINITY) lowest = fminf(lowest, s);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    M = fmaxf(M, __shfl_xor(M, o));
    lowest = fminf(lowest, __shfl_xor(lowest, o));
  }
  if (lane == 0) { pk[wave] = M; ps[wave] = lowest; }
  __syncthreads();
  M = fmaxf(fmaxf(pk[0], pk[1]), fmaxf(pk[2], pk[3]));
  lowest = fminf(fminf(ps[0], ps[1]), fminf(ps[2], ps[3]));
  __syncthreads();
  if (!(M > -INFINITY)) {                              // nothing to pick
    if (tid == 0) {
      if (tok) tok[row] = 0;
      if (ids) ids[(long)row * ld] = 0;
      if (logp) logp[(long)row * ld] = -INFINITY;
    }
    return;
  }

  float S[1] = {0.f};
  for (int v = tid; v < V; v += kNucThreads) S[0] += expf(at(v) - M);     // expf(-inf) = 0: what is not pickable adds nothing
  nuc_sum(S, part);
  const float edge = __fmul_rn(top_p, S[0]);

  // the smallest x in [lo, hi] with sum{e_v : c(v) > (x << shift | ones)} < edge; the caller knows it holds at hi
  auto search = [&](unsigned long long lo, unsigned long long hi, int shift) {
    const unsigned long long ones = (1ull << shift) - 1;
    while (lo < hi) {
      unsigned long long c[kNucCand];
      float a[kNucCand];
#pragma unroll
      for (int j = 0; j < kNucCand; ++j) {             // lo <= c[0] <= ... <= c[14] <= hi - 1
        c[j] = ((lo + (hi - lo) * (unsigned)(j + 1) / (kNucCand + 1)) << shift) | ones;
        a[j] = 0.f;
      }
      for (int v = tid; v < V; v += kNucThreads) {
        const float s = at(v), e = expf(s - M);
        const unsigned long long ck = nuc_ckey(s, v);
#pragma unroll
        for (int j = 0; j < kNucCand; ++j) a[j] += ck > c[j] ? e : 0.f;
      }
      nuc_sum(a, part);
      bool found = false;
#pragma unroll
      for (int j = 0; j < kNucCand; ++j) {             // the first candidate that holds bounds hi, the one before it lo
        const unsigned long long xj = c[j] >> shift;
        if (!found) {
          if (a[j] < edge) { hi = xj; found = true; }
          else lo = xj + 1;
        }
      }
    }
    return hi;
  };
  const unsigned K = (unsigned)search(nuc_key(lowest), nuc_key(M), 24);
  float ties[1] = {0.f};                               // (a count below 2^24: exact in fp32)
  for (int v = tid; v < V; v += kNucThreads) {
    const float s = at(v);
    ties[0] += (s > -INFINITY && nuc_key(s) == K) ? 1.f : 0.f;
  }
  nuc_sum(ties, part);
  unsigned long long cut = (unsigned long long)K << 24;
  if (ties[0] > 1.f) cut = search(cut, cut | 0xffffffull, 0);

  // the draw over the kept entries and their mass
  float kept[1] = {0.f}, bk = -INFINITY, bs = -INFINITY;
  int bi = kVocNone;
  for (int v = tid; v < V; v += kNucThreads) {
    const float s = at(v);
    if (!(s > -INFINITY) || nuc_ckey(s, v) < cut) continue;
    kept[0] += expf(s - M);
    const float key = vs_row_key(s, seed, step, row0 + (unsigned)row, greedy_stride, (unsigned)v);
    if (vocab_better(key, v, bk, bi)) { bk = key; bi = v; bs = s; }
  }
  nuc_sum(kept, part);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bk, o), os = __shfl_xor(bs, o);
    const int oi = __shfl_xor(bi, o);
    if (vocab_better(ov, oi, bk, bi)) { bk = ov; bi = oi; bs = os; }
  }
  if (lane == 0) { pk[wave] = bk; pi[wave] = bi; ps[wave] = bs; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kNucWaves; ++w)
      if (vocab_better(pk[w], pi[w], bk, bi)) { bk = pk[w]; bi = pi[w]; bs = ps[w]; }
    if (tok) tok[row] = bi;
    if (ids) ids[(long)row * ld] = bi;
    if (logp) logp[(long)row * ld] = bs - (M + logf(kept[0]));
  }
}

// one thread per row over the row's k candidates (k <= 16), walked in the total order
__global__ __launch_bounds__(256) void nucleus_pick_kernel(const float* __restrict__ values, const int* __restrict__ index, int rows,
                                                           int k, int V, float inv_T, float top_p, unsigned long long seed,
                                                           unsigned step, unsigned row0, unsigned greedy_stride,
                                                           long long* __restrict__ tok, long long* __restrict__ ids,
                                                           float* __restrict__ logp, long ld) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= rows) return;
  const float* val = values + (long)row * k;
  const int* idx = index + (long)row * k;
  // the best pickable candidate strictly worse than (ps, pv); false: none
  auto next = [&](float ps, int pv, float& ns, int& nv) {
    ns = -INFINITY;
    nv = kVocNone;
    for (int j = 0; j < k; ++j) {
      const int v = idx[j];
      const float s = vs_scaled(val[j], inv_T);
      if (v < 0 || v >= V || !(s > -INFINITY)) continue;      // padding, or nothing to pick
      if (vocab_better(ps, pv, s, v) && vocab_better(s, v, ns, nv)) { ns = s; nv = v; }
    }
    return nv != kVocNone;
  };
  float s = INFINITY, M = -INFINITY, S = 0.f;            // (+inf, -1): better than every candidate
  int v = -1;
  while (next(s, v, s, v)) {
    if (!(M > -INFINITY)) M = s;                           // the first one is the best
    S += expf(s - M);
  }
  const float edge = __fmul_rn(top_p, S);
  float kept = 0.f, bk = -INFINITY, bs = -INFINITY;
  int bi = kVocNone;
  s = INFINITY;
  v = -1;
  while (kept < edge && next(s, v, s, v)) {              // kept is before(v) of the candidate that comes next
    kept += expf(s - M);
    const float key = vs_row_key(s, seed, step, row0 + (unsigned)row, greedy_stride, (unsigned)v);
    if (vocab_better(key, v, bk, bi)) { bk = key; bi = v; bs = s; }
  }
  const bool none = bi == kVocNone;
  const long long t = none ? 0 : bi;
  if (tok) tok[row] = t;
  if (ids) ids[(long)row * ld] = t;
  if (logp) logp[(long)row * ld] = none ? -INFINITY : bs - (M + logf(kept));
}

int nucleus_rows(const float* logits, int rows, long ld_logits, int V, float inv_T, float top_p, unsigned long long seed,
                 unsigned step, unsigned row0, long long* tok, long long* ids, float* logp, long ld, hipStream_t stream,
                 unsigned greedy_stride) {
  CAPNET_REQUIRE(rows >= 1 && V >= 1 && V <= (1 << 24) && ld_logits >= V, "nucleus_rows: rows %d, V %d, ld %ld", rows, V, ld_logits);
  CAPNET_REQUIRE(top_p > 0.f && top_p < 1.f, "nucleus_rows: top_p %g (0 < top_p < 1)", (double)top_p);
  const size_t lds = V <= kNucLdsEntries ? (size_t)V * sizeof(float) : 0;
  hipLaunchKernelGGL(nucleus_rows_kernel, dim3(rows), dim3(kNucThreads), lds, stream, logits, ld_logits, V, inv_T, top_p, seed, step,
                     row0, greedy_stride, tok, ids, logp, ld);
  CAPNET_LAUNCH_CHECK();
  return kOk;
}

int nucleus_pick(const float* values, const int* index, int rows, int k, int V, float inv_T, float top_p, unsigned long long seed,
                 unsigned step, unsigned row0, long long* tok, long long* ids, float* logp, long ld, hipStream_t stream,
                 unsigned greedy_stride) {
  CAPNET_REQUIRE(rows >= 1 && k >= 1 && k <= 16 && V >= 1, "nucleus_pick: rows %d, k %d, V %d", rows, k, V);
  CAPNET_REQUIRE(top_p > 0.f && top_p < 1.f, "nucleus_pick: top_p %g (0 < top_p < 1)", (double)top_p);
  hipLaunchKernelGGL(nucleus_pick_kernel, dim3((rows + 255) / 256), dim3(256), 0, stream, values, index, rows, k, V, inv_T, top_p,
                     seed, step, row0, greedy_stride, tok, ids, logp, ld);
  CAPNET_LAUNCH_CHECK();
  return kOk;
}

}  // namespace capnet
