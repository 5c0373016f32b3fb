// The UNet handle and its packed weights: what unet_build.hip fills and unet.hip runs.
#pragma once

#include "runtime.h"

struct ldmseg_unet;

namespace ldmseg::rt {

inline constexpr int kBlockOut[4] = {320, 640, 1280, 1280};
inline constexpr int kTimeDim = 1280;

struct TransformerW {
  int C = 0;
  NormW norm, ln1, ln3;
  ConvW proj_in, qkv, attn_out, ff1, ff2, proj_out;
  ConvW ffp;                    // bf16, levels without the row-local fused kernel: ff.net.2 and proj_out as ONE Linear over [g | h] (round 5)
  void* mlp_stream = nullptr;   // 320-channel level, bf16: the feed-forward's weights as one consumption-ordered stream (tfuse.hip)
  void* in_stream = nullptr;    // the same for proj_in | to_q | to_k | to_v (tproj.hip)
  float* in_bias = nullptr;     // [4][C]: proj_in bias | W_q beta | W_k beta | W_v beta
  // cross-attention handles (ldmseg_unet_cfg::cross_attention = 1): h = attn2(norm2(h), ctx) + h after attn1
  NormW ln2;
  ConvW q2;                     // to_q with norm2 folded in (c1 / bias as ConvW qkv)
  ConvW kv2;                    // to_k | to_v [2C][768], no bias: applied to the context once per call
  ConvW out2;                   // to_out.0, applied with h as the residual
};
inline constexpr int kCrossDim = 768;        // cross_attention_dim of the SD-1.x UNet
inline constexpr int kHidProjIn = 1024;      // encoder_hid_proj: CLIP-L/14 patch features -> kCrossDim
inline constexpr int kTransformers = 16;

// what the ABI's ldmseg_unet is
struct UnetHandle : HandleBase {
  ldmseg_unet_cfg cfg{};
  float *te1_w = nullptr, *te1_b = nullptr, *te2_w = nullptr, *te2_b = nullptr;
  float *tproj_w = nullptr, *tproj_b = nullptr;
  int temb_total = 0;
  ConvW conv_in, conv_out;
  NormW norm_out;
  ResnetW down_res[4][2], mid_res[2], up_res[4][3];
  TransformerW down_attn[3][2], mid_attn, up_attn[4][3];  // up_attn[0] unused
  ConvW down_conv[3], up_conv[3];
  // cross-attention: optional encoder_hid_proj (1024 -> 768) and where the context's K|V of the running call went
  ConvW hid_proj;
  int ctx_S = 77, ctx_dim = kCrossDim; // shape the workspace is planned for (last call's; 77 text tokens before any call)
  bool ctx_kv_ready = false;           // ldmseg_sample_loop_guided: the context's K|V is already in the workspace (first step made it)
  const void* ctx_kv_base = nullptr;   // workspace base that K|V lives in
  float* guide_buf = nullptr;          // guided loop: [2B,4,L,L] latents | [2B,4,L,L] rgb latents
  size_t guide_elems = 0;
  // sampler state
  int attn_fp8_min_tokens = 0;   // > 0: bf16 mode runs attention levels with N >= this many tokens on the fp8 operand path
  float* cond = nullptr;   // [B,4,L,L] self-conditioning channel
  float* eps = nullptr;
  size_t loop_elems = 0;
  // sampling loops: the time-embedding rows of ALL steps (they depend on the timestep only) from one pass over the
  // 100 MB of time_emb_proj weights instead of one pass per step
  void* temb_buf = nullptr;            // [steps] int64 timesteps | sinusoid | two MLP activations | [steps][temb_total] rows
  int temb_cap = 0;                    // steps the buffer holds
  // fused step tail (tail.hip): a forward whose conv_out launch carried out the scheduler step (UnetCall::tail) leaves the next
  // forward's packed input in place
  bool xin_ready = false;
  const void* xin_ptr = nullptr;       // where the tail wrote that input: the next forward skips its pack only if its own xin IS this buffer
  // Cooperative GroupNorm back-off: the fallback counter of the handle's hand-off region is copied to this
  // pinned word at the end of every sampling call; a call that finds it has grown since the last look runs its norms with a
  // 2 us poll bound (partners that are not co-resident - another process or stream holding CUs - then cost the extra reads of
  // the two-launch scheme instead of a 100 us spin per norm) for the next few calls, then tries the full bound again.
  unsigned long long* gn_diag_host = nullptr;
  unsigned long long gn_diag_seen = 0;
  int gn_backoff_calls = 0;
  // Separate image encoder (unet.py:42-63, 309-351: separate_encoder, optionally add_adaptor): conv_in_img and a copy of the down blocks
  // run on the RGB latents with emb(timestep_img); their 12 outputs (through adaptor_layers[block] where the checkpoint has them) are
  // added to the 12 skip connections.  They depend on the RGB latents and timestep_img only, so a sampling loop computes them once.
  bool sepenc = false, adaptor = false;
  ConvW conv_in_img, adapt[4], img_conv[3];
  ResnetW img_res[4][2];
  TransformerW img_attn[3][2];
  float *tproj_img_w = nullptr, *tproj_img_b = nullptr;
  int temb_img_total = 0;
  void* img_resid = nullptr;           // the 12 residual tensors back to back (handle-owned: the workspace offsets of a forward do not
  size_t img_resid_bytes = 0;          // depend on whether the branch ran in it)
  bool img_ready = false;              // inside ldmseg_sample_loop: a forward with UnetCall::img_keep computed them, they stand

  ~UnetHandle() {
    DeviceGuard dg(device);
    if (cond) (void)hipFree(cond);
    if (eps) (void)hipFree(eps);
    if (temb_buf) (void)hipFree(temb_buf);
    if (gn_diag_host) (void)hipHostFree(gn_diag_host);
    if (guide_buf) (void)hipFree(guide_buf);
    if (img_resid) (void)hipFree(img_resid);
  }
};

// every parameter of the state dict, repacked for the kernels (create time)
int unet_build(ldmseg_unet* u, const WeightMap& wm);

}  // namespace ldmseg::rt

struct ldmseg_unet : ldmseg::rt::UnetHandle {};
