// Policy-gradient loss over a packed batch of sampled captions (self-critical sequence training, Rennie et al. 2017):
//   loss = -(1/N) sum_i adv[cap(i)] * (logit[i][target_i] - lse_i)          N packed rows, B captions
// cap(i): the caption of packed row i. Rows are in pack_padded_sequence order, so in step t (first row off[t]) it is
// i - off[t]; the step offsets ride in the kernel arguments (PolicySteps) and no per-row weight vector exists anywhere.
// Row kernels like xent_fwd_kernel / xent_bwd_kernel of loss_optim.hip, HBM/L2-bound, and in their order of operations
// (max, sum of expf(x - m), the block reductions of block_reduce.h; the final sum in mean_kernel's order): with every
// advantage 1.0f the loss and dlogits are those of xent_fwd / xent_bwd to the last bit (1 x and fma(1, x, a) are exact).
#include "common.h"
#include "kernels.h"
#include "block_reduce.h"
#include "seq_layers.h"

namespace capnet {

struct PolicySteps { int off[kMaxSteps + 1]; int steps; };

// the step of packed row `row`: off[t] <= row < off[t + 1]
__device__ __forceinline__ int policy_step_of(const PolicySteps& st, int row, int t) {
  while (t + 1 < st.steps && row >= st.off[t + 1]) ++t;
  return t;
}

// one workgroup per row: lse[row] = log sum exp, row_logp[row] = logit[target] - lse
__global__ __launch_bounds__(256) void policy_xent_fwd_kernel(const float* __restrict__ logits, long ld, int V,
                                                              const long long* __restrict__ target,
                                                              float* __restrict__ lse, float* __restrict__ row_logp,
                                                              int* __restrict__ err_flag) {
  __shared__ float s[4];
  const int row = blockIdx.x;
  const float* p = logits + (long)row * ld;
  float m = -INFINITY;
  for (int j = threadIdx.x; j < V; j += blockDim.x) m = fmaxf(m, p[j]);
  m = block_reduce_max(m, s);
  float z = 0.f;
  for (int j = threadIdx.x; j < V; j += blockDim.x) z += expf(p[j] - m);
  z = block_reduce_sum(z, s);
  if (threadIdx.x == 0) {
    const float l = m + logf(z);
    lse[row] = l;
    const long long t = target[row];
    if (t < 0 || t >= V) {
      atomicOr(err_flag, 2);
      row_logp[row] = 0.f;
    } else {
      row_logp[row] = -(l - p[t]);   // xent_fwd_kernel's row loss, negated
    }
  }
}

// loss = sum_i adv[cap(i)] * -row_logp[i] / N by a single workgroup, thread k taking rows k, k + 256, ... as mean_kernel
// does. A row of advantage 0 adds nothing, whatever its logits were.
__global__ __launch_bounds__(256) void policy_loss_kernel(const float* __restrict__ row_logp, const float* __restrict__ adv,
                                                          PolicySteps st, int n, float* __restrict__ out) {
  __shared__ float s[4];
  float a = 0.f;
  int t = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    t = policy_step_of(st, i, t);
    const float w = adv[i - st.off[t]];
    if (w != 0.f) a += w * -row_logp[i];
  }
  a = block_reduce_sum(a, s);
  if (threadIdx.x == 0) out[0] = a / (float)n;
}

// caption_logp[b] = sum of caption b's rows in step order: one thread per caption, one fixed order, no atomics
__global__ __launch_bounds__(64) void policy_caption_logp_kernel(const float* __restrict__ row_logp, PolicySteps st, int B,
                                                                 float* __restrict__ caption_logp) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float a = 0.f;
  for (int t = 0; t < st.steps && b < st.off[t + 1] - st.off[t]; ++t) a += row_logp[st.off[t] + b];
  caption_logp[b] = a;
}

static int policy_steps(const char* who, const int* batch_sizes, int steps, int B, int N, PolicySteps* st) {
  CAPNET_REQUIRE(steps > 0 && steps <= kMaxSteps, "%s: %d steps (1..%d)", who, steps, kMaxSteps);
  CAPNET_REQUIRE(batch_sizes && batch_sizes[0] == B, "%s: batch_sizes[0] must be the %d captions", who, B);
  RC(seqd::check_batch_sizes(who, batch_sizes, steps, B, N));
  st->steps = steps;
  st->off[0] = 0;
  for (int t = 0; t < steps; ++t) st->off[t + 1] = st->off[t] + batch_sizes[t];
  for (int t = steps + 1; t <= kMaxSteps; ++t) st->off[t] = N;
  return kOk;
}

int policy_xent_fwd(const float* logits, long ld, int N, int V, const long long* targets, const float* adv, int B,
                    const int* batch_sizes, int steps, float* lse, float* row_logp, float* caption_logp, float* loss,
                    int* err_flag, hipStream_t stream) {
  CAPNET_REQUIRE(logits && targets && adv && lse && row_logp && caption_logp && loss && err_flag && N > 0 && V > 0 &&
                     B > 0 && ld >= V,
                 "policy_xent_fwd: bad argument");
  PolicySteps st;
  RC(policy_steps("policy_xent_fwd", batch_sizes, steps, B, N, &st));
  hipLaunchKernelGGL(policy_xent_fwd_kernel, dim3(N), dim3(256), 0, stream, logits, ld, V, targets, lse, row_logp,
                     err_flag);
  hipLaunchKernelGGL(policy_loss_kernel, dim3(1), dim3(256), 0, stream, row_logp, adv, st, N, loss);
  hipLaunchKernelGGL(policy_caption_logp_kernel, dim3(cdiv(B, 64)), dim3(64), 0, stream, row_logp, st, B, caption_logp);
  CAPNET_LAUNCH_CHECK();
  return kOk;
}

// dlogits[row][j] = (softmax - onehot) * (gout[0] / N * adv[cap(row)]), the factor formed once per row. A row of
// advantage 0 (under the greedy baseline: every sample equal to the greedy caption) writes zeros without reading its logits.
__global__ __launch_bounds__(256) void policy_xent_bwd_kernel(const float* __restrict__ logits, long ld, int V,
                                                              const long long* __restrict__ target,
                                                              const float* __restrict__ lse, const float* __restrict__ adv,
                                                              PolicySteps st, const float* __restrict__ gout, float inv_n,
                                                              float* __restrict__ dlogits, long ldd) {
  const int row = blockIdx.x;
  float* d = dlogits + (long)row * ldd;
  const float w = adv[row - st.off[policy_step_of(st, row, 0)]];
  if (w == 0.f) {
    for (int j = threadIdx.x; j < V; j += blockDim.x) d[j] = 0.f;
    return;
  }
  const float* p = logits + (long)row * ld;
  const float l = lse[row];
  const float g = gout[0] * inv_n * w;
  const long long t = target[row];
  for (int j = threadIdx.x; j < V; j += blockDim.x) {
    float v = expf(p[j] - l);
    if (j == t) v -= 1.f;
    d[j] = v * g;
  }
}

int policy_xent_bwd(const float* logits, long ld, int N, int V, const long long* targets, const float* lse,
                    const float* adv, int B, const int* batch_sizes, int steps, const float* gout, float* dlogits,
                    long ldd, hipStream_t stream) {
  CAPNET_REQUIRE(logits && targets && lse && adv && gout && dlogits && N > 0 && V > 0 && B > 0 && ld >= V && ldd >= V,
                 "policy_xent_bwd: bad argument");
  PolicySteps st;
  RC(policy_steps("policy_xent_bwd", batch_sizes, steps, B, N, &st));
  hipLaunchKernelGGL(policy_xent_bwd_kernel, dim3(N), dim3(256), 0, stream, logits, ld, V, targets, lse, adv, st, gout,
                     1.f / (float)N, dlogits, ldd);
  CAPNET_LAUNCH_CHECK();
  return kOk;
}

}  // namespace capnet
