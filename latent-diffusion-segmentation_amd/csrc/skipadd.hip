// dst = a + b over up to 12 dense tensors in ONE launch: the separate image encoder's residuals added to the UNet's skip
// connections (unet.py:375-385) between the down path and the mid block.
//
// Pure streaming: 16 bytes per lane per access (8 bf16 / 4 fp32), blocks of 256, the grid capped at 8 blocks per CU and
// grid-striding over ONE flat index of 16-byte units that runs through all segments, so that a small segment does not get a
// launch - or a tail of idle lanes - of its own.  The sum is formed in fp32 and rounded once to the storage type.  No LDS, no
// atomics.  A segment whose pointers are not 16-byte aligned, and the last partial unit of a segment whose length is not a multiple
// of the unit, go element by element.  dst may be a or b (every lane reads its unit before it writes it).
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"

namespace ldmseg {
namespace {

struct SkipAddArgs {
  SkipAddSeg seg[kSkipAddMaxSegs];
  long long first[kSkipAddMaxSegs + 1];   // flat index of a segment's first unit; first[n] = units in all
  int vec[kSkipAddMaxSegs];               // dst, a and b are 16-byte aligned
  int n;
};

template <typename T>
__global__ __launch_bounds__(256) void skip_add_kernel(const SkipAddArgs A) {
  constexpr int V = Chunk<T>::N;
  const long long stride = (long long)gridDim.x * 256;
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  for (int k = 0; k < A.n; ++k) {          // (uniform: the segment's pointers are scalar loads)
    T* dst = (T*)A.seg[k].dst;
    const T* a = (const T*)A.seg[k].a;
    const T* b = (const T*)A.seg[k].b;
    const long long elems = A.seg[k].elems, base = A.first[k], end = A.first[k + 1];
    const bool vec = A.vec[k] != 0;
    for (; i < end; i += stride) {
      const long long e0 = (i - base) * V;
      if (vec && e0 + V <= elems) {
        const uint4 ca = *reinterpret_cast<const uint4*>(a + e0);
        const uint4 cb = *reinterpret_cast<const uint4*>(b + e0);
        float fa[V], fb[V];
        Chunk<T>::unpack(ca, fa);
        Chunk<T>::unpack(cb, fb);
#pragma unroll
        for (int j = 0; j < V; ++j) fa[j] += fb[j];
        *reinterpret_cast<uint4*>(dst + e0) = Chunk<T>::pack(fa);
      } else {
        for (int j = 0; j < V && e0 + j < elems; ++j) dst[e0 + j] = from_f32<T>(to_f32<T>(a[e0 + j]) + to_f32<T>(b[e0 + j]));
      }
    }
  }
}

}  // namespace

int launch_skip_add(const SkipAddSeg* segs, int n_segs, int dtype, hipStream_t s) {
  if (!segs || n_segs < 1 || n_segs > kSkipAddMaxSegs || (dtype != DT_BF16 && dtype != DT_F32)) return -2;
  const int V = dtype == DT_BF16 ? 8 : 4;
  SkipAddArgs A{};
  A.n = n_segs;
  long long units = 0;
  for (int k = 0; k < n_segs; ++k) {
    if (!segs[k].dst || !segs[k].a || !segs[k].b || segs[k].elems < 0) return -2;
    A.seg[k] = segs[k];
    A.first[k] = units;
    A.vec[k] = (((uintptr_t)segs[k].dst | (uintptr_t)segs[k].a | (uintptr_t)segs[k].b) & 15) == 0;
    units += (segs[k].elems + V - 1) / V;
  }
  A.first[n_segs] = units;
  if (units == 0) return 0;
  const long long cap = (long long)num_cus() * 8;
  const long long want = (units + 255) / 256;
  const int grid = (int)(want < cap ? want : cap);
  if (dtype == DT_BF16)
    LDMSEG_LAUNCH(launch_name("skip_add<%s>", dtype_tag<bf16_t>()), skip_add_kernel<bf16_t>, dim3(grid), dim3(256), 0, s, A);
  else
    LDMSEG_LAUNCH(launch_name("skip_add<%s>", dtype_tag<float>()), skip_add_kernel<float>, dim3(grid), dim3(256), 0, s, A);
  return launch_status();
}

}  // namespace ldmseg
