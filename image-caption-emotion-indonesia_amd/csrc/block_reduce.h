// Max and sum over a workgroup of whole waves (at most four): a wave-64 butterfly, one LDS slot per wave, then every thread
// adds the slots in wave order. One copy, so the row kernels of loss_optim.hip and policy_loss.hip reduce in the same order
// and agree to the last bit where they compute the same thing; caption_reward.hip sums its integer counts the same way.
#pragma once
#include "common.h"

namespace capnet {

__device__ __forceinline__ float block_reduce_max(float v, float* s) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = s[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r = fmaxf(r, s[w]);
  __syncthreads();
  return r;
}
__device__ __forceinline__ float block_reduce_sum(float v, float* s) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = s[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r += s[w];
  __syncthreads();
  return r;
}
// the same for integer counts (caption_reward.hip): exact in any order
__device__ __forceinline__ int block_reduce_sum(int v, int* s) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = s[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r += s[w];
  __syncthreads();
  return r;
}
// and for fp64 terms (caption_reward.hip's CIDEr-D sums): the same butterfly, so the order of the additions is fixed by the
// thread index alone and two launches on the same input agree to the last bit
__device__ __forceinline__ double block_reduce_sum(double v, double* s) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = s[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r += s[w];
  __syncthreads();
  return r;
}

}  // namespace capnet
