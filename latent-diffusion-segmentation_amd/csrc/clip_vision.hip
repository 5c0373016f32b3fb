// Row-local kernels of the CLIP ViT image encoder (transformers CLIPVisionModel / CLIPVisionModelWithProjection, the image
// descriptor of the clip_image / clip_image_proj modes).  Everything between them - the patch GEMM, the folded-LayerNorm
// q|k|v and fc1 GEMMs, out_proj / fc2 with the residual in the epilogue, head-dim-64 self-attention - runs on the kernels
// of igemm.hip / attention.hip; the executor that strings them together is the clip-vision section of engine.hip.
//
//   clip_patch_rows   image -> the patch conv's GEMM operand [B * G * G][Kpad], k = (channel, dy, dx) in the conv weight's own
//                     order, K zero-padded to whole 128-byte lines.  RESAMPLE: norm_resize_images fused in front
//                     (F.interpolate bilinear, align_corners=False, no antialias, then (x - mean) / std).
//   clip_tokens       [class_embedding | patch rows] + position_embedding, then pre_layrnorm -> the residual stream.
//   clip_pooled_ln    post_layernorm of the class-token row of every image -> fp32 [B][C] (feeds launch_small_linear).
//   clip_rows_to_f32  residual stream -> the fp32 last_hidden_state at the API boundary.
#include "common.h"
#include "kernels.h"

namespace ldmseg {
namespace {

struct ClipFront {
  const float* img;       // [B][3][H][W] fp32
  int H, W, S, P, G, K, Kpad;
  float ry, rx;           // H / S, W / S in fp32 (torch's area_pixel_compute_scale)
  float mean[3], std[3];
  FastDiv fd_pp, fd_p, fd_gg, fd_g;
};

template <typename T, bool RESAMPLE>
__global__ __launch_bounds__(256) void clip_patch_rows_kernel(ClipFront f, T* __restrict__ rows) {
  const int row = blockIdx.x;                           // (image, gy, gx)
  const int b = fd_div(row, f.fd_gg), cell = row - b * f.G * f.G;
  const int gy = fd_div(cell, f.fd_g), gx = cell - gy * f.G;
  T* out = rows + (size_t)row * f.Kpad;
  for (int k = threadIdx.x; k < f.Kpad; k += 256) {
    float v = 0.f;
    if (k < f.K) {
      const int c = fd_div(k, f.fd_pp), r = k - c * f.P * f.P;
      const int dy = fd_div(r, f.fd_p), dx = r - dy * f.P;
      const int y = gy * f.P + dy, x = gx * f.P + dx;
      const float* plane = f.img + ((size_t)b * 3 + c) * f.H * f.W;
      if constexpr (RESAMPLE) {
        // torch upsample_bilinear2d, align_corners=False: src = max(0, scale * (dst + 0.5) - 0.5), the neighbour clamped at the edge.
        // Every operation is spelled out in the order and with the fused multiply-adds of torch's CPU kernel (lerp(t0, w0, t1, w1) =
        // fma(t0, w0, t1 * w1), along x then along y; the source index itself one fma), so that the fp32 rows agree with
        // F.interpolate bit for bit and the bf16 rows round the same number - a value next to zero has no slack for an fp32 ulp.
        const float sy = fmaxf(__fmaf_rn(f.ry, __fadd_rn((float)y, 0.5f), -0.5f), 0.f);
        const float sx = fmaxf(__fmaf_rn(f.rx, __fadd_rn((float)x, 0.5f), -0.5f), 0.f);
        const int y0 = min((int)sy, f.H - 1), x0 = min((int)sx, f.W - 1);
        const int y1 = y0 + (y0 < f.H - 1 ? 1 : 0), x1 = x0 + (x0 < f.W - 1 ? 1 : 0);
        const float ly = fminf(fmaxf(__fsub_rn(sy, (float)y0), 0.f), 1.f), lx = fminf(fmaxf(__fsub_rn(sx, (float)x0), 0.f), 1.f);
        const float hy = __fsub_rn(1.f, ly), hx = __fsub_rn(1.f, lx);
        const float a = plane[(size_t)y0 * f.W + x0], bb = plane[(size_t)y0 * f.W + x1];
        const float cc = plane[(size_t)y1 * f.W + x0], d = plane[(size_t)y1 * f.W + x1];
        const float top = __fmaf_rn(a, hx, __fmul_rn(bb, lx)), bot = __fmaf_rn(cc, hx, __fmul_rn(d, lx));
        v = __fmaf_rn(top, hy, __fmul_rn(bot, ly));
        v = __fdiv_rn(__fsub_rn(v, f.mean[c]), f.std[c]);
      } else {
        v = plane[(size_t)y * f.W + x];
      }
    }
    out[k] = from_f32<T>(v);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void clip_tokens_kernel(const T* __restrict__ patch, const float* __restrict__ cls,
                                                          const float* __restrict__ pos, const float* __restrict__ g,
                                                          const float* __restrict__ bt, T* __restrict__ h, int T_, int C, float eps) {
  __shared__ float red[4];
  const int row = blockIdx.x;                           // image * T + token
  const int b = row / T_, t = row - b * T_;
  float v[kClipMaxPer];
#pragma unroll
  for (int i = 0; i < kClipMaxPer; ++i) {
    const int c = threadIdx.x + i * 256;
    v[i] = 0.f;
    if (c < C) v[i] = (t == 0 ? cls[c] : to_f32<T>(patch[((size_t)b * (T_ - 1) + (t - 1)) * C + c])) + pos[(size_t)t * C + c];
  }
  row_layernorm<kClipMaxPer>(v, C, eps, g, bt, red);
#pragma unroll
  for (int i = 0; i < kClipMaxPer; ++i) { const int c = threadIdx.x + i * 256; if (c < C) h[(size_t)row * C + c] = from_f32<T>(v[i]); }
}

template <typename T>
__global__ __launch_bounds__(256) void clip_pooled_ln_kernel(const T* __restrict__ h, const float* __restrict__ g,
                                                             const float* __restrict__ bt, float* __restrict__ out, int T_, int C,
                                                             float eps) {
  __shared__ float red[4];
  const int b = blockIdx.x;
  const T* r = h + (size_t)b * T_ * C;                  // the class-token row
  float v[kClipMaxPer];
#pragma unroll
  for (int i = 0; i < kClipMaxPer; ++i) { const int c = threadIdx.x + i * 256; v[i] = c < C ? to_f32<T>(r[c]) : 0.f; }
  row_layernorm<kClipMaxPer>(v, C, eps, g, bt, red);
#pragma unroll
  for (int i = 0; i < kClipMaxPer; ++i) { const int c = threadIdx.x + i * 256; if (c < C) out[(size_t)b * C + c] = v[i]; }
}

template <typename T>
__global__ __launch_bounds__(256) void clip_rows_to_f32_kernel(const T* __restrict__ x, float* __restrict__ y, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) y[i] = to_f32<T>(x[i]);
}


}  // namespace

int launch_clip_patch_rows(const float* img, void* rows, int B, int H, int W, int S, int P, int Kpad, const float* mean,
                           const float* std, int resample, int dtype, hipStream_t s) {
  if (B < 1 || H < 1 || W < 1 || P < 1 || S < P || S % P != 0 || Kpad < 3 * P * P) return -2;
  if (!resample && (H != S || W != S)) return -2;
  if (resample && (!mean || !std)) return -2;
  ClipFront f;
  f.img = img; f.H = H; f.W = W; f.S = S; f.P = P; f.G = S / P; f.K = 3 * P * P; f.Kpad = Kpad;
  f.ry = (float)H / (float)S; f.rx = (float)W / (float)S;
  for (int c = 0; c < 3; ++c) { f.mean[c] = mean ? mean[c] : 0.f; f.std[c] = std ? std[c] : 1.f; }
  f.fd_pp = fastdiv_make(P * P); f.fd_p = fastdiv_make(P); f.fd_gg = fastdiv_make(f.G * f.G); f.fd_g = fastdiv_make(f.G);
  const dim3 grid((unsigned)(B * f.G * f.G));
  auto k_b1 = clip_patch_rows_kernel<bf16_t, true>;
  auto k_b0 = clip_patch_rows_kernel<bf16_t, false>;
  auto k_f1 = clip_patch_rows_kernel<float, true>;
  auto k_f0 = clip_patch_rows_kernel<float, false>;
  const std::string name = launch_name("clip_patch_rows<%s,%d>", dtype == DT_BF16 ? "bf16" : "f32", resample ? 1 : 0);
  if (dtype == DT_BF16) LDMSEG_LAUNCH(name, resample ? k_b1 : k_b0, grid, dim3(256), 0, s, f, (bf16_t*)rows);
  else LDMSEG_LAUNCH(name, resample ? k_f1 : k_f0, grid, dim3(256), 0, s, f, (float*)rows);
  return launch_status();
}

int launch_clip_tokens(const void* patch, const float* cls, const float* pos, const float* gamma, const float* beta, void* h,
                       int B, int T, int C, float eps, int dtype, hipStream_t s) {
  if (B < 1 || T < 2 || C < 1 || C > 256 * kClipMaxPer) return -2;
  const dim3 grid((unsigned)(B * T));
  if (dtype == DT_BF16)
    LDMSEG_LAUNCH(launch_name("clip_tokens<%s>", "bf16"), clip_tokens_kernel<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)patch, cls, pos,
                  gamma, beta, (bf16_t*)h, T, C, eps);
  else
    LDMSEG_LAUNCH(launch_name("clip_tokens<%s>", "f32"), clip_tokens_kernel<float>, grid, dim3(256), 0, s, (const float*)patch, cls, pos,
                  gamma, beta, (float*)h, T, C, eps);
  return launch_status();
}

int launch_clip_pooled_ln(const void* h, const float* gamma, const float* beta, float* out, int B, int T, int C, float eps,
                          int dtype, hipStream_t s) {
  if (B < 1 || T < 1 || C < 1 || C > 256 * kClipMaxPer) return -2;
  if (dtype == DT_BF16)
    LDMSEG_LAUNCH(launch_name("clip_pooled_ln<%s>", "bf16"), clip_pooled_ln_kernel<bf16_t>, dim3(B), dim3(256), 0, s, (const bf16_t*)h, gamma,
                  beta, out, T, C, eps);
  else
    LDMSEG_LAUNCH(launch_name("clip_pooled_ln<%s>", "f32"), clip_pooled_ln_kernel<float>, dim3(B), dim3(256), 0, s, (const float*)h, gamma,
                  beta, out, T, C, eps);
  return launch_status();
}

int launch_clip_rows_to_f32(const void* x, float* y, size_t n, int dtype, hipStream_t s) {
  if (n == 0) return 0;
  size_t blocks = (n + 255) / 256;
  const dim3 grid((unsigned)(blocks < 8192 ? blocks : 8192));
  if (dtype == DT_BF16)
    LDMSEG_LAUNCH(launch_name("clip_rows_to_f32<%s>", "bf16"), clip_rows_to_f32_kernel<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)x, y, n);
  else
    LDMSEG_LAUNCH(launch_name("clip_rows_to_f32<%s>", "f32"), clip_rows_to_f32_kernel<float>, grid, dim3(256), 0, s, (const float*)x, y, n);
  return launch_status();
}

}  // namespace ldmseg
