// Fixed-order workgroup sum and the order-preserving fp32 radix key: what the element loss (loss.hip) and both directions of
// the point loss (point_loss_dev.h) share.  Device code, included by files compiled with -ffp-contract=off.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace ldmseg {

constexpr int kBlockSumThreads = 256;              // workgroup size block_sum is written for (its includers assert theirs)

// sum over the workgroup in a fixed order: lanes by xor-shuffle tree, then the four waves in order; valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* s_red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();                                 // s_red may still be read from a previous call
  if (lane == 0) s_red[wave] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < kBlockSumThreads / 64; ++w) t += s_red[w];
  return t;
}

// order-preserving key of an fp32 bit pattern (larger value <-> larger key; the losses are non-negative, the map also orders
// negative values should a caller hand some in)
__device__ __forceinline__ uint32_t f32_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_f32(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

}  // namespace ldmseg
