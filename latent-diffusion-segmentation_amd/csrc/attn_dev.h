// Device helpers the LDS-DMA attention kernels share (attention3.hip, attention4.hip, attention_fp8.hip).
#pragma once
#include "common.h"

namespace ldmseg {

// smallest bf16-representable value >= x (finite x), returned as f32
__device__ __forceinline__ float bf16_ceil(float x) {
  const uint32_t u = f32_bits(x);
  return bits_f32(((u & 0x80000000u) ? u : u + 0xffffu) & 0xffff0000u);
}
// LDS-DMA of 64 x 16 B: lane l fetches gsrc(l) + OFF into LDS lds_dst + 16 l.  The instruction's immediate offset is
// applied to the global AND the LDS address, so M0 carries lds_dst - OFF (callers keep lds_dst >= OFF).
template <int OFF>
__device__ __forceinline__ void glds16_off(const void* gsrc, unsigned lds_dst) {
  asm volatile(
      "s_mov_b32 m0, %1\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %0, off offset:%2"
      :
      : "v"(gsrc), "s"(lds_dst - OFF), "i"(OFF)
      : "memory");
}
template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"i"(N) : "memory");
}

}  // namespace ldmseg
