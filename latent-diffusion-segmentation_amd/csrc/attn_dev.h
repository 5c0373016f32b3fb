// Device helpers the LDS-DMA attention kernels share (attention3.hip, attention4.hip, attention_fp8.hip, attention_mx.hip);
// the LDS-DMA primitives themselves are in lds_dma.h.
#pragma once
#include "common.h"
#include "lds_dma.h"

namespace ldmseg {

// smallest bf16-representable value >= x (finite x), returned as f32
__device__ __forceinline__ float bf16_ceil(float x) {
  const uint32_t u = f32_bits(x);
  return bits_f32(((u & 0x80000000u) ? u : u + 0xffffu) & 0xffff0000u);
}
__device__ __forceinline__ float clamp448(float x) { return fminf(fmaxf(x, -448.f), 448.f); }
// four floats -> one dword of e4m3 (RNE; inputs must be within +-448)
__device__ __forceinline__ uint32_t pack_fp8x4(float a, float b, float c, float d) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
  return (uint32_t)w;
}
__device__ __forceinline__ float fp8_to_f32(uint32_t byte) { return __builtin_amdgcn_cvt_f32_fp8((int)byte, 0); }

}  // namespace ldmseg
