// The reward of decoded captions on the device, from the ids the samplers leave in memory: sentence BLEU (capnet_bleu_rows) or
// CIDEr-D (capnet_cider_rows) of every row of a sampled decode against its image's references. Both kernels share one
// staging of a row (stage_row: the hypothesis rule and the image's references in LDS) and one n-gram comparison (bleu_same).
//   hyp(row)  = [start] + ids[row][0 .. j], j the first column holding end_token (none: all `steps` columns), L words
// BLEU, capnet.metrics.corpus_bleu of ONE sentence:
//   num_n     = sum over the DISTINCT n-grams g of hyp of min(count of g in hyp, max over references of its count there)
//   den_n     = max(1, L - n + 1)
//   closest   = the reference length nearest to L, ties to the shorter
//   bp        = 1 if L > closest, else exp(1 - closest / L)
//   reward    = bp exp(sum_n w_n log(num_n / den_n)),  0 where any num_n is 0
//   smooth 1  (Lin & Och 2004, add one): (num_n + 1) / (den_n + 1) for n >= 2; 0 only where num_1 is 0
// One workgroup per row; thread p owns hypothesis position p (L <= 129). Brute force: the n-gram at p is counted where no
// earlier position holds the same one -- in the hypothesis and in every reference, by comparison -- and min(count, max) is
// summed over the workgroup as an integer (block_reduce.h: exact in any order). No atomics, no hash table, no sort. The
// image's references sit in LDS (at most kBleuRefWords words). One thread forms the score in fp64 and rounds it once.
// Columns behind the first end_token do not enter anything. A reference slot of length 0 is absent.
// CIDEr-D (Vedantam et al. 2015, the COCO tools' cider_scorer; capnet.metrics.cider_d_parts), per order n = 1..4:
//   idf(g)    = the value the host stored for g in order n's sorted key table, log_n where the table does not hold g
//   v_s(g)    = (count of g in s) * idf(g);   norm_n(s) = sqrt(sum_g v_s(g)^2) -- of a reference: read from ref_norm
//   sim_n(r)  = sum over the distinct g of hyp of min(v_h(g), v_r(g)) v_r(g) / (norm_n(hyp) norm_n(r))  (0 norms: undivided)
//               times exp(-(L - len r)^2 / (2 sigma^2))
//   part_n    = the mean of sim_n over the image's non-empty references;   reward = 2.5 (part_1 + .. + part_4)
// The same thread-per-position brute force; the thread that owns a distinct n-gram finds its idf by binary search on whole
// n-word keys (exact: no hash, no probing; the table is only read). All terms are fp64 and are summed over the workgroup
// by block_reduce.h's fixed butterfly, so two launches agree bit for bit. Threads at or beyond L, and threads whose n-gram
// occurred earlier, add exact zeros.
#include "common.h"
#include "kernels.h"
#include "block_reduce.h"

namespace capnet {

constexpr int kBleuThreads = 256;

struct RowArgs {            // what both kernels stage of a row
  const long long* ids;     // [rows][ld]
  long ld;
  int steps, per_image, R, Lr;
  long long start, end;
  const int* refs;          // [images][R][Lr]
  const int* ref_len;       // [images][R]
};

struct BleuArgs : RowArgs {
  int smooth;
  double w[4];
  float* reward;            // [rows]
  int* stats;               // [rows][10]
};

struct CiderArgs : RowArgs {
  const double* ref_norm;   // [images][R][4]
  const int* keys[4];       // order n: [count[n - 1]][n], ascending
  const double* idf[4];     // order n: [count[n - 1]]
  int count[4];
  double log_n, sigma;
  float* reward;            // [rows]
  double* parts;            // [rows][4]
  int* stats;               // [rows][9]
};

template <class T>
__device__ __forceinline__ bool bleu_same(const T* a, const long long* b, int n) {
  bool eq = true;
  for (int j = 0; j < n; ++j) eq = eq && (long long)a[j] == b[j];
  return eq;
}

// The hypothesis rule, and the image's references: hyp[0 .. L) = [start] + the row's ids through the first end (none: all
// `steps` columns), ref / rlen the reference slots of image row / per_image (a length clamped into [0, Lr]). Returns L to
// every thread; both barriers are inside.
__device__ __forceinline__ int stage_row(const RowArgs& a, long long* hyp, int* ref, int* rlen, int* hlen) {
  const int row = blockIdx.x, tid = threadIdx.x, R = a.R, Lr = a.Lr;
  const long img = row / a.per_image;
  if (tid == 0) hyp[0] = a.start;
  if (tid < a.steps) hyp[tid + 1] = a.ids[(long)row * a.ld + tid];
  for (int i = tid; i < R * Lr; i += kBleuThreads) ref[i] = a.refs[img * R * Lr + i];
  if (tid < R) rlen[tid] = min(max(a.ref_len[img * R + tid], 0), Lr);
  __syncthreads();
  if (tid == 0) {
    int L = a.steps + 1;
    for (int t = 1; t <= a.steps; ++t)
      if (hyp[t] == a.end) { L = t + 1; break; }
    *hlen = L;
  }
  __syncthreads();
  return *hlen;
}

__global__ __launch_bounds__(kBleuThreads) void bleu_rows_kernel(BleuArgs a) {
  __shared__ long long hyp[kBleuMaxSteps + 1];
  __shared__ int ref[kBleuRefWords];
  __shared__ int rlen[kBleuMaxRefs];
  __shared__ int red[kBleuThreads / 64];
  __shared__ int hlen;
  const int row = blockIdx.x, tid = threadIdx.x, R = a.R, Lr = a.Lr;
  const int L = stage_row(a, hyp, ref, rlen, &hlen), p = tid;
  int num[4];
  for (int n = 1; n <= 4; ++n) {
    int add = 0;
    if (p + n <= L) {
      bool first = true;
      for (int q = 0; q < p && first; ++q) first = !bleu_same(hyp + q, hyp + p, n);
      if (first) {
        int ch = 1, mx = 0;
        for (int q = p + 1; q + n <= L; ++q) ch += bleu_same(hyp + q, hyp + p, n) ? 1 : 0;
        for (int r = 0; r < R; ++r) {
          int c = 0;
          for (int q = 0; q + n <= rlen[r]; ++q) c += bleu_same(ref + r * Lr + q, hyp + p, n) ? 1 : 0;
          mx = max(mx, c);
        }
        add = min(ch, mx);
      }
    }
    num[n - 1] = block_reduce_sum(add, red);
  }
  if (tid != 0) return;
  int closest = 0, gap = 0;
  bool any = false;
  for (int r = 0; r < R; ++r) {          // the nearest length, ties to the shorter
    const int rl = rlen[r], g = abs(rl - L);
    if (rl > 0 && (!any || g < gap || (g == gap && rl < closest))) { closest = rl; gap = g; any = true; }
  }
  int* st = a.stats + (long)row * 10;
  bool zero = num[0] == 0;
  double s = 0.0;
  for (int n = 1; n <= 4; ++n) {
    const int den = max(1, L - n + 1);
    st[n - 1] = num[n - 1];
    st[3 + n] = den;
    const int up = a.smooth && n >= 2 ? 1 : 0;
    if (num[n - 1] + up == 0) zero = true;
    else s += a.w[n - 1] * log((double)(num[n - 1] + up) / (double)(den + up));
  }
  st[8] = L;
  st[9] = closest;
  const double bp = L > closest ? 1.0 : exp(1.0 - (double)closest / (double)L);
  a.reward[row] = zero ? 0.f : (float)(bp * exp(s));
}

int bleu_rows(const long long* ids, long ld, int rows, int steps, long long start_token, long long end_token, int per_image,
              const int* refs, const int* ref_len, int images, int R, int Lr, const double* weights, int smooth, float* reward,
              int* stats, hipStream_t stream) {
  CAPNET_REQUIRE(ids && refs && ref_len && weights && reward && stats, "bleu_rows: null argument");
  CAPNET_REQUIRE(rows >= 1 && steps >= 1 && steps <= kBleuMaxSteps && ld >= steps, "bleu_rows: rows %d, steps %d (1..%d), ld %ld", rows,
                 steps, kBleuMaxSteps, ld);
  CAPNET_REQUIRE(R >= 1 && R <= kBleuMaxRefs && Lr >= 1 && (long)R * Lr <= kBleuRefWords,
                 "bleu_rows: %d references of %d words (at most %d references, %d words in all)", R, Lr, kBleuMaxRefs, kBleuRefWords);
  CAPNET_REQUIRE(per_image >= 1 && images >= 1 && (long)rows <= (long)images * per_image,
                 "bleu_rows: %d rows, %d per image, references of %d images", rows, per_image, images);
  CAPNET_REQUIRE(smooth == 0 || smooth == 1, "bleu_rows: smooth %d (0 or 1)", smooth);
  BleuArgs a;
  a.ids = ids; a.ld = ld; a.steps = steps; a.per_image = per_image; a.R = R; a.Lr = Lr; a.smooth = smooth;
  a.start = start_token; a.end = end_token; a.refs = refs; a.ref_len = ref_len;
  for (int n = 0; n < 4; ++n) a.w[n] = weights[n];
  a.reward = reward; a.stats = stats;
  hipLaunchKernelGGL(bleu_rows_kernel, dim3(rows), dim3(kBleuThreads), 0, stream, a);
  CAPNET_LAUNCH_CHECK();
  return kOk;
}

// idf of the n-gram g in the sorted table (keys [count][n], ascending by whole key): binary search, every word compared.
// *hit says whether the table holds g; where it does not, the caller's miss value comes back.
__device__ __forceinline__ double cider_idf(const int* keys, const double* idf, int count, const long long* g, int n, double miss,
                                            bool* hit) {
  int lo = 0, hi = count;                 // the answer, if any, is in [lo, hi)
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    const int* k = keys + (long)mid * n;
    int cmp = 0;                          // sign of key - g, decided at the first word that differs
    for (int j = 0; j < n && cmp == 0; ++j) {
      const long long kw = k[j];
      cmp = kw < g[j] ? -1 : (kw > g[j] ? 1 : 0);
    }
    if (cmp == 0) { *hit = true; return idf[mid]; }
    if (cmp < 0) lo = mid + 1;
    else hi = mid;
  }
  *hit = false;
  return miss;
}

__global__ __launch_bounds__(kBleuThreads) void cider_rows_kernel(CiderArgs a) {
  __shared__ long long hyp[kBleuMaxSteps + 1];
  __shared__ int ref[kBleuRefWords];
  __shared__ int rlen[kBleuMaxRefs];
  __shared__ double red[kBleuThreads / 64];
  __shared__ int redi[kBleuThreads / 64];
  __shared__ int hlen;
  const int row = blockIdx.x, tid = threadIdx.x, R = a.R, Lr = a.Lr;
  const long img = row / a.per_image;
  const int L = stage_row(a, hyp, ref, rlen, &hlen), p = tid;
  double part[4];
  int seen[4];                            // distinct_n + (known_n << 16): both at most 129
  for (int n = 1; n <= 4; ++n) {
    bool first = false, hit = false;
    double vh = 0.0, idf = 0.0;
    if (p + n <= L) {
      first = true;
      for (int q = 0; q < p && first; ++q) first = !bleu_same(hyp + q, hyp + p, n);
      if (first) {
        int ch = 1;
        for (int q = p + 1; q + n <= L; ++q) ch += bleu_same(hyp + q, hyp + p, n) ? 1 : 0;
        idf = cider_idf(a.keys[n - 1], a.idf[n - 1], a.count[n - 1], hyp + p, n, a.log_n, &hit);
        vh = (double)ch * idf;
      }
    }
    seen[n - 1] = block_reduce_sum(first ? 1 + (hit ? 1 << 16 : 0) : 0, redi);
    const double norm_h = sqrt(block_reduce_sum(vh * vh, red));
    double sum = 0.0;
    int refs_used = 0;
    for (int r = 0; r < R; ++r) {         // R and rlen are the same for every thread: so are the barriers inside
      if (rlen[r] == 0) continue;
      double term = 0.0;
      if (first) {
        int c = 0;
        for (int q = 0; q + n <= rlen[r]; ++q) c += bleu_same(ref + r * Lr + q, hyp + p, n) ? 1 : 0;
        const double vr = (double)c * idf;
        term = fmin(vh, vr) * vr;
      }
      const double raw = block_reduce_sum(term, red);
      if (tid == 0) {
        const double norm_r = a.ref_norm[(img * R + r) * 4 + (n - 1)];
        const double d = (double)(L - rlen[r]);
        const double sim = norm_h != 0.0 && norm_r != 0.0 ? raw / (norm_h * norm_r) : raw;
        sum += sim * exp(-(d * d) / (2.0 * a.sigma * a.sigma));
      }
      ++refs_used;
    }
    part[n - 1] = refs_used ? sum / (double)refs_used : 0.0;
  }
  if (tid != 0) return;
  int* st = a.stats + (long)row * 9;
  st[0] = L;
  for (int n = 0; n < 4; ++n) {
    st[1 + n] = seen[n] & 0xffff;
    st[5 + n] = seen[n] >> 16;
    a.parts[(long)row * 4 + n] = part[n];
  }
  a.reward[row] = (float)(2.5 * (part[0] + part[1] + part[2] + part[3]));
}

int cider_rows(const long long* ids, long ld, int rows, int steps, long long start_token, long long end_token, int per_image,
               const int* refs, const int* ref_len, const double* ref_norm, int images, int R, int Lr, const int* const* keys,
               const double* const* idf, const int* counts, double log_n, double sigma, float* reward, double* parts, int* stats,
               hipStream_t stream) {
  CAPNET_REQUIRE(ids && refs && ref_len && ref_norm && keys && idf && counts && reward && parts && stats, "cider_rows: null argument");
  CAPNET_REQUIRE(rows >= 1 && steps >= 1 && steps <= kBleuMaxSteps && ld >= steps, "cider_rows: rows %d, steps %d (1..%d), ld %ld", rows,
                 steps, kBleuMaxSteps, ld);
  CAPNET_REQUIRE(R >= 1 && R <= kBleuMaxRefs && Lr >= 1 && (long)R * Lr <= kBleuRefWords,
                 "cider_rows: %d references of %d words (at most %d references, %d words in all)", R, Lr, kBleuMaxRefs, kBleuRefWords);
  CAPNET_REQUIRE(per_image >= 1 && images >= 1 && (long)rows <= (long)images * per_image,
                 "cider_rows: %d rows, %d per image, references of %d images", rows, per_image, images);
  CAPNET_REQUIRE(sigma > 0.0, "cider_rows: sigma %g (must be positive)", sigma);
  CiderArgs a;
  a.ids = ids; a.ld = ld; a.steps = steps; a.per_image = per_image; a.R = R; a.Lr = Lr;
  a.start = start_token; a.end = end_token; a.refs = refs; a.ref_len = ref_len; a.ref_norm = ref_norm;
  for (int n = 0; n < 4; ++n) {
    CAPNET_REQUIRE(counts[n] >= 0 && (counts[n] == 0 || (keys[n] && idf[n])), "cider_rows: order %d, %d keys (a null table only at 0)",
                   n + 1, counts[n]);
    a.keys[n] = keys[n]; a.idf[n] = idf[n]; a.count[n] = counts[n];
  }
  a.log_n = log_n; a.sigma = sigma;
  a.reward = reward; a.parts = parts; a.stats = stats;
  hipLaunchKernelGGL(cider_rows_kernel, dim3(rows), dim3(kBleuThreads), 0, stream, a);
  CAPNET_LAUNCH_CHECK();
  return kOk;
}

}  // namespace capnet
