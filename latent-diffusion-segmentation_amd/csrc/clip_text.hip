// Row-local kernels of the CLIP text encoder (transformers CLIPTextModel, SD-1.x's text_encoder: the conditioning model of
// image_descriptors `none`, ldmseg/models/descriptors.py:98-103, called at trainers_ldm_cond.py:1108-1119).  The layers between
// them run on the kernels the vision tower uses (the folded-LayerNorm q|k|v and fc1 GEMMs, out_proj / fc2 with the residual in
// the epilogue) and on the causal form of the head-dim-64 self-attention in attention.hip; the executor is the clip-text section
// of engine.hip.
//
//   clip_text_tokens    h[r][t] = token_embedding[ids[r][t]] + position_embedding[t] -> the residual stream (fp32 sum, one rounding)
//   clip_text_final_ln  final_layer_norm of every row of the residual stream -> the fp32 last_hidden_state at the API boundary
#include "common.h"
#include "kernels.h"

namespace ldmseg {
namespace {

template <typename T>
__global__ __launch_bounds__(256) void clip_text_tokens_kernel(const int64_t* __restrict__ ids, const float* __restrict__ tok,
                                                               const float* __restrict__ pos, T* __restrict__ h, int T_, int C,
                                                               int vocab) {
  const int row = blockIdx.x;                           // prompt * T + position
  const int t = row % T_;
  // clamped for memory safety only: the caller checks the range (an id outside [0, vocab) is an IndexError in the Python wrapper)
  int64_t id = ids[row];
  id = id < 0 ? 0 : (id >= vocab ? (int64_t)vocab - 1 : id);
  const float* e = tok + (size_t)id * C;
  const float* p = pos + (size_t)t * C;
  for (int c = threadIdx.x; c < C; c += 256) h[(size_t)row * C + c] = from_f32<T>(e[c] + p[c]);
}

template <typename T>
__global__ __launch_bounds__(256) void clip_text_final_ln_kernel(const T* __restrict__ h, const float* __restrict__ g,
                                                                 const float* __restrict__ bt, float* __restrict__ out, int C,
                                                                 float eps) {
  __shared__ float red[4];
  const size_t row = blockIdx.x;
  float v[kClipMaxPer];
#pragma unroll
  for (int i = 0; i < kClipMaxPer; ++i) { const int c = threadIdx.x + i * 256; v[i] = c < C ? to_f32<T>(h[row * C + c]) : 0.f; }
  row_layernorm<kClipMaxPer>(v, C, eps, g, bt, red);
#pragma unroll
  for (int i = 0; i < kClipMaxPer; ++i) { const int c = threadIdx.x + i * 256; if (c < C) out[row * C + c] = v[i]; }
}


}  // namespace

int launch_clip_text_tokens(const int64_t* ids, const float* tok, const float* pos, void* h, int R, int T, int C, int vocab,
                            int dtype, hipStream_t s) {
  if (R < 1 || T < 1 || C < 1 || vocab < 1) return -2;
  const dim3 grid((unsigned)(R * T));
  if (dtype == DT_BF16)
    LDMSEG_LAUNCH(launch_name("clip_text_tokens<%s>", "bf16"), clip_text_tokens_kernel<bf16_t>, grid, dim3(256), 0, s, ids, tok, pos,
                  (bf16_t*)h, T, C, vocab);
  else
    LDMSEG_LAUNCH(launch_name("clip_text_tokens<%s>", "f32"), clip_text_tokens_kernel<float>, grid, dim3(256), 0, s, ids, tok, pos,
                  (float*)h, T, C, vocab);
  return launch_status();
}

int launch_clip_text_final_ln(const void* h, const float* gamma, const float* beta, float* out, int M, int C, float eps, int dtype,
                              hipStream_t s) {
  if (M < 1 || C < 1 || C > 256 * kClipMaxPer) return -2;
  if (dtype == DT_BF16)
    LDMSEG_LAUNCH(launch_name("clip_text_final_ln<%s>", "bf16"), clip_text_final_ln_kernel<bf16_t>, dim3(M), dim3(256), 0, s,
                  (const bf16_t*)h, gamma, beta, out, C, eps);
  else
    LDMSEG_LAUNCH(launch_name("clip_text_final_ln<%s>", "f32"), clip_text_final_ln_kernel<float>, dim3(M), dim3(256), 0, s,
                  (const float*)h, gamma, beta, out, C, eps);
  return launch_status();
}

}  // namespace ldmseg
