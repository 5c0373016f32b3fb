// Cross-attention core of a diffusers BasicTransformerBlock (attn2: queries from the image tokens, keys / values from a short
// conditioning context - 77 CLIP text tokens, 257 CLIP-L/14 patch features, or one projected image embedding).
//
// out[b, n, head*d + i] = sum_j softmax_j(q[b,n,head] . k[b,j,head] * d^-1/2) v[b,j,head][i]
//   q   [B*N, C]   the to_q GEMM's output
//   kv  [B*S, 2C]  to_k | to_v of the context (k at columns [0, C), v at [C, 2C)), channel = head*d + i
//   out [B*N, C]
//
// The launch streams Q once and writes the output once; its arithmetic is small (2 S d multiply-adds per query row and head,
// S <= a few hundred), so every product runs in fp32 on the VALU whatever the storage type: bf16 tensors are widened on load,
// fp32 tensors (the exact and the split-bf16 modes) are used as they are.  One workgroup = 64 query rows of one (image, head);
// four lanes share a row (d / 4 dimensions each, the dot product finished by two quad DPP adds).  Keys are walked in LDS
// tiles of 32 with the online softmax of attention.hip (running max in the log2 domain, rescale of the accumulator per tile);
// keys past S are masked in the tile loop, so any S >= 1 works without padding.
#include <hip/hip_runtime.h>

#include "attn_plan.h"
#include "common.h"
#include "kernels.h"

namespace ldmseg {
namespace {

constexpr int kRows = 64;      // query rows per workgroup (4 lanes each: 256 threads)
constexpr int kKeys = 32;      // keys per LDS tile

template <typename T, int D>
__global__ __launch_bounds__(256) void attention_cross_kernel(const T* __restrict__ q, const T* __restrict__ kv,
                                                              T* __restrict__ out, int N, int S, int C, float qscale) {
  constexpr int DQ = D / 4;                          // dimensions per lane
  constexpr int W = (DQ % 4 == 0) ? 4 : 2;           // LDS vector width (DQ = 10: 8-byte reads)
  typedef float fv __attribute__((ext_vector_type(W)));
  __shared__ __attribute__((aligned(16))) float ks[kKeys * D];
  __shared__ __attribute__((aligned(16))) float vs[kKeys * D];
  const int tid = threadIdx.x;
  const int part = tid & 3;
  const int row = blockIdx.x * kRows + (tid >> 2);
  const int head = blockIdx.y;
  const int b = blockIdx.z;
  const bool live = row < N;

  float qr[DQ], acc[DQ];
  {
    const T* qp = q + ((size_t)b * N + (live ? row : 0)) * C + head * D + part * DQ;
#pragma unroll
    for (int i = 0; i < DQ; ++i) {
      qr[i] = live ? to_f32<T>(qp[i]) * qscale : 0.f;     // d^-1/2 * log2(e) folded into q
      acc[i] = 0.f;
    }
  }
  float m = -INFINITY, l = 0.f;
  const T* kvb = kv + (size_t)b * S * 2 * C + head * D;
  for (int t0 = 0; t0 < S; t0 += kKeys) {
    const int nk = S - t0 < kKeys ? S - t0 : kKeys;
    __syncthreads();
    for (int e = tid; e < kKeys * D; e += 256) {
      const int j = e / D, i = e - j * D;
      float kx = 0.f, vx = 0.f;
      if (j < nk) {
        const T* r = kvb + (size_t)(t0 + j) * 2 * C + i;
        kx = to_f32<T>(r[0]);
        vx = to_f32<T>(r[C]);
      }
      ks[e] = kx;
      vs[e] = vx;
    }
    __syncthreads();
    float sc[kKeys];
    float mt = m;
#pragma unroll
    for (int j = 0; j < kKeys; ++j) {
      sc[j] = -INFINITY;
      if (j < nk) {                                  // (nk is uniform over the workgroup: the DPP lanes are all active)
        const fv* kr = reinterpret_cast<const fv*>(ks + j * D + part * DQ);
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < DQ / W; ++c) {
          const fv x = kr[c];
#pragma unroll
          for (int w = 0; w < W; ++w) dot = fmaf(qr[c * W + w], x[w], dot);
        }
        dot += dpp_f<0xB1>(dot);                     // quad_perm [1,0,3,2]
        dot += dpp_f<0x4E>(dot);                     // quad_perm [2,3,0,1]
        sc[j] = dot;
        mt = fmaxf(mt, dot);
      }
    }
    const float corr = exp2f(m - mt);                // first tile: exp2(-inf) = 0
    l *= corr;
#pragma unroll
    for (int i = 0; i < DQ; ++i) acc[i] *= corr;
#pragma unroll
    for (int j = 0; j < kKeys; ++j) {
      if (j < nk) {
        const float p = exp2f(sc[j] - mt);
        l += p;
        const fv* vr = reinterpret_cast<const fv*>(vs + j * D + part * DQ);
#pragma unroll
        for (int c = 0; c < DQ / W; ++c) {
          const fv x = vr[c];
#pragma unroll
          for (int w = 0; w < W; ++w) acc[c * W + w] = fmaf(p, x[w], acc[c * W + w]);
        }
      }
    }
    m = mt;
  }
  if (live) {
    const float inv = 1.f / l;
    T* op = out + ((size_t)b * N + row) * C + head * D + part * DQ;
#pragma unroll
    for (int i = 0; i < DQ; ++i) op[i] = from_f32<T>(acc[i] * inv);
  }
}

template <typename T>
__global__ void rows_to_dtype_kernel(const float* __restrict__ x, T* __restrict__ y, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = from_f32<T>(x[i]);
}

template <typename T, int D>
int launch_d(const AttnPlan& p, const void* q, const void* kv, void* out, hipStream_t s) {
  static_assert(kRows == kAttnCrossRows, "attn_plan.h sizes the grid from it");
  const float qscale = 1.4426950408889634f / sqrtf((float)D);
  LDMSEG_LAUNCH(launch_name("attention_cross_kernel<%s,%d>", dtype_tag<T>(), D), (attention_cross_kernel<T, D>),
                dim3(p.grid_x, p.grid_y, p.grid_z), dim3(p.block), 0, s, (const T*)q, (const T*)kv, (T*)out, p.q.N, p.q.S, p.q.C, qscale);
  return launch_status();
}

template <typename T>
int dispatch(const AttnPlan& p, const void* q, const void* kv, void* out, hipStream_t s) {
  switch (p.D) {
    case 40: return launch_d<T, 40>(p, q, kv, out, s);
    case 80: return launch_d<T, 80>(p, q, kv, out, s);
    case 160: return launch_d<T, 160>(p, q, kv, out, s);
    default: return -2;
  }
}

}  // namespace

int launch_attn_cross_plan(const AttnPlan& p, const void* q, const void* kv, void* out, hipStream_t s) {
  if (p.form != ATTN_CROSS) return -2;
  return p.q.dtype == DT_BF16 ? dispatch<bf16_t>(p, q, kv, out, s)
                              : dispatch<float>(p, q, kv, out, s);      // (dtype 2: fp32 tensors of a bf16x3 handle)
}

int launch_attention_cross(const void* q, const void* kv, void* out, int B, int N, int S, int C, int heads, int dtype,
                           hipStream_t s) {
  AttnPlan p;
  if (attn_choose(AttnDesc{ATTN_KIND_CROSS, B, N, S, C, heads, dtype}, attention_knobs(), &p)) return -2;
  return launch_attn_cross_plan(p, q, kv, out, s);
}

int launch_rows_to_dtype(const float* x, void* y, size_t n, int dtype, hipStream_t s) {
  const dim3 grid((unsigned)((n + 255) / 256));
  if (dtype == DT_BF16)
    LDMSEG_LAUNCH(launch_name("rows_to_dtype_kernel<%s>", "bf16"), rows_to_dtype_kernel<bf16_t>, grid, dim3(256), 0, s, x,
                  (bf16_t*)y, n);
  else
    LDMSEG_LAUNCH(launch_name("rows_to_dtype_kernel<%s>", "f32"), rows_to_dtype_kernel<float>, grid, dim3(256), 0, s, x,
                  (float*)y, n);
  return launch_status();
}

}  // namespace ldmseg
