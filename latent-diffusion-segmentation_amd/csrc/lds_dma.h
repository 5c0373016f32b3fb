// LDS-DMA and its waits: the one copy of the inline-asm primitives that igemm.hip, tfuse.hip, tproj.hip, tail.hip and the
// attention kernels issue.  A hazard fix (wait state, clobber list) is made here and nowhere else.
#pragma once
#include <hip/hip_runtime.h>

namespace ldmseg {

// LDS-DMA: 64 lanes x 16 B from per-lane global addresses into LDS at (wave-uniform) lds_dst +
// lane*16.  Issued through inline asm so that hipcc does not track it: with the builtin the
// compiler waits vmcnt(0) before the next ds_read (it cannot prove the DMA target and the tile
// being read are different stages), which serialises DMA and MFMA.  The caller owns the wait:
// s_waitcnt vmcnt(0) + barrier before any wave reads the stage.
__device__ __forceinline__ void glds16(const void* gsrc, unsigned lds_dst) {
  asm volatile(
      "s_mov_b32 m0, %1\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %0, off"
      :
      : "v"(gsrc), "s"(lds_dst)
      : "memory");
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
// same as glds16, address = wave-uniform 64-bit base (SGPR pair) + per-lane 32-bit offset: no VALU per tile
__device__ __forceinline__ void glds16_sbase(unsigned voff, const void* sbase, unsigned lds_dst) {
  asm volatile(
      "s_mov_b32 m0, %2\n\t"
      "s_nop 3\n\t"   // M0 write -> LDS-DMA needs 1 wait state; an SGPR base written by SALU / v_readfirstlane needs 5
                       // before a VMEM instruction reads it, and the hazard recognizer does not look inside inline asm
                       // (a register-load variant of this helper went to wild addresses without them)
      "global_load_lds_dwordx4 %0, %1"
      :
      : "v"(voff), "s"(sbase), "s"(lds_dst)
      : "memory");
}
// two consecutive pieces (2 KiB) from one base: the instruction's immediate offset moves the LDS address along with the global
// one (wait states as in glds16_sbase)
__device__ __forceinline__ void glds16x2_sbase(unsigned voff, const void* sbase, unsigned lds_dst) {
  asm volatile(
      "s_mov_b32 m0, %2\n\t"
      "s_nop 3\n\t"
      "global_load_lds_dwordx4 %0, %1\n\t"
      "global_load_lds_dwordx4 %0, %1 offset:1024"
      :
      : "v"(voff), "s"(sbase), "s"(lds_dst)
      : "memory");
}

// at most N of this wave's vector-memory operations (LDS-DMA pieces included) still in flight
template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"i"(N) : "memory");
}
// the same for a run-time n: at most n of this wave's LDS-DMA pieces still in flight (n <= 16: the wave's share of the ring)
__device__ __forceinline__ void wait_pieces(int n) {
  switch (n) {
#define LDMSEG_WAIT_VM(N) case N: asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory"); break;
    LDMSEG_WAIT_VM(0) LDMSEG_WAIT_VM(1) LDMSEG_WAIT_VM(2) LDMSEG_WAIT_VM(3) LDMSEG_WAIT_VM(4) LDMSEG_WAIT_VM(5)
    LDMSEG_WAIT_VM(6) LDMSEG_WAIT_VM(7) LDMSEG_WAIT_VM(8) LDMSEG_WAIT_VM(9) LDMSEG_WAIT_VM(10) LDMSEG_WAIT_VM(11)
    LDMSEG_WAIT_VM(12) LDMSEG_WAIT_VM(13) LDMSEG_WAIT_VM(14) LDMSEG_WAIT_VM(15)
#undef LDMSEG_WAIT_VM
    default: asm volatile("s_waitcnt vmcnt(16)" ::: "memory"); break;
  }
}

// workgroup barrier that waits for this wave's LDS traffic only (what __syncthreads() compiles to on gfx950 outside tgsplit mode;
// spelled out because the compute waves must never wait for vmcnt here: their epilogue stores are still in flight)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

}  // namespace ldmseg
