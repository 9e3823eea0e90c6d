// The reward of decoded captions on the device: sentence BLEU of every row of a sampled decode against its image's
// references (capnet_bleu_rows), from the ids the samplers leave in memory. capnet.metrics.corpus_bleu of ONE sentence:
//   hyp(row)  = [start] + ids[row][0 .. j], j the first column holding end_token (none: all `steps` columns), L words
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
#include "common.h"
#include "kernels.h"
#include "block_reduce.h"

namespace capnet {

constexpr int kBleuThreads = 256;

struct BleuArgs {
  const long long* ids;     // [rows][ld]
  long ld;
  int steps, per_image, R, Lr, smooth;
  long long start, end;
  const int* refs;          // [images][R][Lr]
  const int* ref_len;       // [images][R]
  double w[4];
  float* reward;            // [rows]
  int* stats;               // [rows][10]
};

template <class T>
__device__ __forceinline__ bool bleu_same(const T* a, const long long* b, int n) {
  bool eq = true;
  for (int j = 0; j < n; ++j) eq = eq && (long long)a[j] == b[j];
  return eq;
}

__global__ __launch_bounds__(kBleuThreads) void bleu_rows_kernel(BleuArgs a) {
  __shared__ long long hyp[kBleuMaxSteps + 1];
  __shared__ int ref[kBleuRefWords];
  __shared__ int rlen[kBleuMaxRefs];
  __shared__ int red[kBleuThreads / 64];
  __shared__ int hlen;
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
    hlen = L;
  }
  __syncthreads();
  const int L = hlen, p = tid;
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

}  // namespace capnet
