// The two VAEs of libldmseg_hip.so with their C ABI (include/ldmseg_hip.h): the seg-VAE (encoder, decoder, the fused evaluation
// tails and the reconstruct chain) and the encoder of SD-1.x's image VAE (AutoencoderKL).  The runtime underneath: runtime.h.
#include <cmath>

#include "runtime.h"
#include "vae_bwd.h"

#pragma clang diagnostic ignored "-Wc++20-designator"      // ConvOpt and its like are filled by field name

using namespace ldmseg;
using namespace ldmseg::rt;

// =================================================================== seg-VAE
struct ldmseg_vae : HandleBase {
  ldmseg_vae_cfg cfg{};
  // encoder
  ConvW enc[10];          // encoder.{0,2,3,5,6,8,9,11,15} in order (9 used)
  NormW enc_gn;
  int enc_ch[5]{};        // storage channel counts
  // decoder
  ConvW dec_in, dec_out;
  ConvW convt[4];
  NormW ln[4], dec_gn;
  // fp32-storage handles: the decoder's convs packed a second time for their data gradients (ldmseg_vae_decode_backward)
  ConvW dec_in_d, dec_out_d, convt_d[4];
  // ... and the encoder's (ldmseg_vae_encode_backward): enc_d[k] for enc[k], k = 1 .. 8 (the first conv's input is data)
  ConvW enc_d[10];
};

// =================================================================== image VAE encoder (AutoencoderKL, SD-1.x)
struct ldmseg_vae_image : HandleBase {
  ldmseg_vae_image_cfg cfg{};
  ConvW conv_in, downs[3], conv_out, quant;
  ResnetW down[4][2], mid[2];
  NormW attn_gn, norm_out;
  ConvW q, k, proj;
  void* wv = nullptr;       // value projection [512][512], used as the X operand of the V^T GEMM
  float* bv = nullptr;
};

namespace {

inline int cstore(int c, int dt) { return (int)rup(c, bke(dt)); }

// ---- the decoder's data-gradient packings: the same igemm reads them as ordinary [N][K] weights
// dX = conv3x3(dY, W transposed and rotated by 180 degrees): N = Ci, K = 9 * Co (Co padded to a K tile)
void dgrad_conv_shape(ConvW* d, int Co, int Ci, int epi) {
  d->N = (int)rup(Ci, igemm_pick_bn(Ci, epi)); d->n_valid = Ci; d->cin_pad = (int)rup(Co, bke(DT_F32)); d->taps = 9; d->cout = Ci;
}
// dX[p] = dY[p, 2x2, :] W[ci][co][q]: N = Ci, K = 4 * Co on the phase-major dY
void dgrad_convt_shape(ConvW* d, int Ci, int Co) {
  d->N = (int)rup(Ci, igemm_pick_bn(Ci, EPI_STORE)); d->n_valid = Ci; d->cin_pad = 4 * Co; d->taps = 1; d->cout = Ci;
}
size_t convw_floats(const ConvW& d) { return (size_t)d.N * d.taps * d.cin_pad; }

// dX of a STRIDE-2 conv3x3 = the four output phases as 4 Ci columns of one 3x3 GEMM over dY, scattered by EPI_CONVT2
void dgrad_conv_s2_shape(ConvW* d, int Co, int Ci) {
  d->N = (int)rup(4 * Ci, igemm_pick_bn(4 * Ci, EPI_CONVT2)); d->n_valid = 4 * Ci; d->cin_pad = (int)rup(Co, bke(DT_F32)); d->taps = 9; d->cout = Ci;
}

// the encoder's nine convs in model order (vae.py:174-244): state-dict index, channels, stride, whether SiLU follows in the epilogue
struct EncLayer { int idx, Co, Ci, stride, silu; };
constexpr int kEncLayers = 9, kEncNormIdx = 13;
std::vector<EncLayer> encoder_layers(const ldmseg_vae_cfg& c) {
  const int* boc = c.block_out_channels;
  std::vector<EncLayer> l;
  l.push_back({0, boc[0], c.in_channels, 1, 1});
  int idx = 2;
  for (int i = 0; i < 3; ++i) {
    l.push_back({idx, boc[i], boc[i], 1, 0});
    l.push_back({idx + 1, boc[i + 1], boc[i], 2, 1});
    idx += 3;
  }
  l.push_back({idx, c.int_channels, boc[3], 1, 0});
  l.push_back({idx + 4, c.latent_channels * c.num_latents, c.int_channels, 1, 0});
  return l;
}

// reference keys of the decoder in model order with their element counts: (conv_in w, b), per upscaler (convT w, b, LayerNorm w, b),
// (GroupNorm w, b), (conv_out w, b)
struct DecKey { std::string name; int64_t numel; };
std::vector<DecKey> decoder_keys(const ldmseg_vae_cfg& c) {
  std::vector<DecKey> k;
  auto add = [&](int idx, int64_t wn, int64_t bn) {
    k.push_back({"decoder." + std::to_string(idx) + ".weight", wn});
    k.push_back({"decoder." + std::to_string(idx) + ".bias", bn});
  };
  add(0, (int64_t)c.int_channels * c.latent_channels * 9, c.int_channels);
  int idx = 2, cin = c.int_channels;
  for (int i = 0; i < c.num_upscalers; ++i) {
    add(idx, (int64_t)cin * c.upscale_channels * 4, c.upscale_channels);
    add(idx + 1, c.upscale_channels, c.upscale_channels);
    cin = c.upscale_channels;
    idx += 3;
  }
  add(idx, cin, cin);
  add(idx + 2, (int64_t)c.out_channels * cin * 9, c.out_channels);
  return k;
}

// ... and of the encoder: (conv w, b) of layers 0 .. 7 at slots 2 k, 2 k + 1, (GroupNorm w, b) at 16, 17, (head w, b) at 18, 19
std::vector<DecKey> encoder_keys(const ldmseg_vae_cfg& c) {
  std::vector<DecKey> k;
  const std::vector<EncLayer> l = encoder_layers(c);
  auto add = [&](int idx, int64_t wn, int64_t bn) {
    k.push_back({"encoder." + std::to_string(idx) + ".weight", wn});
    k.push_back({"encoder." + std::to_string(idx) + ".bias", bn});
  };
  for (int i = 0; i < kEncLayers - 1; ++i) add(l[i].idx, (int64_t)l[i].Co * l[i].Ci * 9, l[i].Co);
  add(l[kEncLayers - 1].idx - 2, c.int_channels, c.int_channels);
  add(l[kEncLayers - 1].idx, (int64_t)l[kEncLayers - 1].Co * l[kEncLayers - 1].Ci * 9, l[kEncLayers - 1].Co);
  return k;
}
constexpr size_t kEncNormSlot = 16, kEncHeadSlot = 18;
inline size_t enc_slot(int k) { return k == kEncLayers - 1 ? kEncHeadSlot : (size_t)2 * k; }

// name -> slot of `keys`, with the checks the backward and the load entries share; -1 and the message set on a bad name or numel
int key_slot(const std::vector<DecKey>& keys, const char* name, int64_t numel, const char* what) {
  size_t k = 0;
  while (name && k < keys.size() && keys[k].name != name) ++k;
  if (!name) fail(LDMSEG_E_ARG, "null tensor name");
  else if (k == keys.size()) fail(LDMSEG_E_ARG, std::string("not ") + what + " parameter: " + name);
  else if (numel != keys[k].numel) fail(LDMSEG_E_ARG, keys[k].name + " has " + std::to_string(keys[k].numel) + " elements, got " + std::to_string(numel));
  else return (int)k;
  return -1;
}

// (Re)packs the encoder tensors `wm` holds into the buffers the handle owns, as vae_pack_decoder does for the decoder's
int vae_pack_encoder(ldmseg_vae* v, const WeightMap& wm, hipStream_t s, bool forward_too) {
  const ldmseg_vae_cfg& c = v->cfg;
  const int dt = v->dt;
  const bool f32 = dt == DT_F32;
  const std::vector<DecKey> keys = encoder_keys(c);
  const std::vector<EncLayer> l = encoder_layers(c);
  auto has = [&](size_t slot, const float** p) {
    auto it = wm.m.find(keys[slot].name);
    if (it == wm.m.end()) return false;
    *p = it->second.first;
    return true;
  };
  auto planes = [&](void* w, size_t nfloats) { return (v->x3 && f32) ? launch_split_planes(w, nfloats, s) : 0; };
  for (int k = 0; k < kEncLayers; ++k) {
    const size_t slot = enc_slot(k);
    ConvW& fw = v->enc[k];
    ConvW& dg = v->enc_d[k];
    const float* p;
    if (has(slot, &p)) {
      if (forward_too) {
        TRY(launch_repack_conv(p, fw.w, l[k].Co, l[k].Ci, 3, 3, fw.N, fw.cin_pad, dt, s));
        TRY(planes(fw.w, convw_floats(fw)));
      }
      if (f32 && dg.w) {
        if (l[k].stride == 2) TRY(launch_pack_dgrad_conv_s2(p, (float*)dg.w, l[k].Co, l[k].Ci, dg.N, dg.cin_pad, s));
        else TRY(launch_pack_dgrad_conv(p, (float*)dg.w, l[k].Co, l[k].Ci, dg.N, dg.cin_pad, s));
        TRY(planes(dg.w, convw_floats(dg)));
      }
    }
    if (forward_too && has(slot + 1, &p)) TRY(launch_padded_bias(p, l[k].Co, fw.bias, fw.N, s));
  }
  const float* p;
  if (forward_too && has(kEncNormSlot, &p)) HIP_TRY(hipMemcpyAsync(v->enc_gn.g, p, c.int_channels * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (forward_too && has(kEncNormSlot + 1, &p)) HIP_TRY(hipMemcpyAsync(v->enc_gn.b, p, c.int_channels * sizeof(float), hipMemcpyDeviceToDevice, s));
  return 0;
}
// the encoder's backward needs every activation width to be its channel count (no padded channels between the layers)
bool encoder_backward_ok(const ldmseg_vae_cfg& c) {
  for (int i = 0; i < 4; ++i)
    if (c.block_out_channels[i] % 32) return false;
  return c.int_channels % 32 == 0 && c.latent_channels * c.num_latents <= 32;
}

// (Re)packs the decoder tensors `wm` holds into the buffers the handle owns - forward packing, data-gradient packing, the hi | lo
// planes of a bf16x3 handle, norm and bias vectors - with the launches the build uses.  Keys that are absent are left alone.
int vae_pack_decoder(ldmseg_vae* v, const WeightMap& wm, hipStream_t s, bool forward_too) {
  const ldmseg_vae_cfg& c = v->cfg;
  const int dt = v->dt;
  const bool f32 = dt == DT_F32;
  const std::vector<DecKey> keys = decoder_keys(c);
  auto has = [&](size_t slot, const float** p) {
    auto it = wm.m.find(keys[slot].name);
    if (it == wm.m.end()) return false;
    *p = it->second.first;
    return true;
  };
  auto planes = [&](void* w, size_t nfloats) { return (v->x3 && f32) ? launch_split_planes(w, nfloats, s) : 0; };
  auto conv3 = [&](size_t slot, ConvW& fw, ConvW& dg, int Co, int Ci) -> int {
    const float* p;
    if (has(slot, &p)) {
      if (forward_too) {
        TRY(launch_repack_conv(p, fw.w, Co, Ci, 3, 3, fw.N, fw.cin_pad, dt, s));
        TRY(planes(fw.w, convw_floats(fw)));
      }
      if (f32) {
        TRY(launch_pack_dgrad_conv(p, (float*)dg.w, Co, Ci, dg.N, dg.cin_pad, s));
        TRY(planes(dg.w, convw_floats(dg)));
      }
    }
    if (forward_too && has(slot + 1, &p)) TRY(launch_padded_bias(p, Co, fw.bias, fw.N, s));
    return 0;
  };
  auto vec = [&](size_t slot, float* dst, int n) -> int {
    const float* p;
    if (forward_too && has(slot, &p)) HIP_TRY(hipMemcpyAsync(dst, p, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    return 0;
  };
  size_t slot = 0;
  TRY(conv3(slot, v->dec_in, v->dec_in_d, c.int_channels, c.latent_channels));
  slot += 2;
  int cin = c.int_channels;
  for (int i = 0; i < c.num_upscalers; ++i) {
    const int Co = c.upscale_channels;
    ConvW& t = v->convt[i];
    const float* p;
    if (has(slot, &p)) {
      if (forward_too) {
        TRY(launch_repack_convt2(p, t.w, cin, Co, dt, s));
        TRY(planes(t.w, (size_t)4 * Co * cin));
      }
      if (f32) {
        TRY(launch_pack_dgrad_convt(p, (float*)v->convt_d[i].w, cin, Co, v->convt_d[i].N, s));
        TRY(planes(v->convt_d[i].w, convw_floats(v->convt_d[i])));
      }
    }
    if (forward_too && has(slot + 1, &p))
      for (int q = 0; q < 4; ++q) HIP_TRY(hipMemcpyAsync(t.bias + q * Co, p, Co * sizeof(float), hipMemcpyDeviceToDevice, s));
    TRY(vec(slot + 2, v->ln[i].g, Co));
    TRY(vec(slot + 3, v->ln[i].b, Co));
    cin = Co;
    slot += 4;
  }
  TRY(vec(slot, v->dec_gn.g, cin));
  TRY(vec(slot + 1, v->dec_gn.b, cin));
  TRY(conv3(slot + 2, v->dec_out, v->dec_out_d, c.out_channels, cin));
  return 0;
}

int vae_build(ldmseg_vae* v, const WeightMap& wm) {
  Builder b(*v, wm);
  hipStream_t s = b.s;
  const ldmseg_vae_cfg& c = v->cfg;
  const int dt = v->dt;
  if (c.in_channels > bke(dt) || c.latent_channels > bke(dt)) return fail(LDMSEG_E_ARG, "too many boundary channels");
  if (c.int_channels % 64 || c.upscale_channels % 64 || c.num_upscalers < 1 || c.num_upscalers > 4)
    return fail(LDMSEG_E_ARG, "unsupported seg-VAE configuration");
  // ---- encoder (vae.py:174-244) ----
  const int* boc = c.block_out_channels;
  int k = 0;
  TRY(b.conv("encoder.0", boc[0], c.in_channels, 3, bke(dt), &v->enc[k++], true, cstore(boc[0], dt)));
  int idx = 2;
  for (int i = 0; i < 3; ++i) {
    TRY(b.conv("encoder." + std::to_string(idx), boc[i], boc[i], 3, cstore(boc[i], dt), &v->enc[k++], true, cstore(boc[i], dt)));
    TRY(b.conv("encoder." + std::to_string(idx + 1), boc[i + 1], boc[i], 3, cstore(boc[i], dt), &v->enc[k++], true,
               cstore(boc[i + 1], dt)));
    idx += 3;
  }
  TRY(b.conv("encoder." + std::to_string(idx), c.int_channels, boc[3], 3, cstore(boc[3], dt), &v->enc[k++]));
  TRY(b.norm("encoder." + std::to_string(idx + 2), c.int_channels, &v->enc_gn));
  TRY(b.conv("encoder." + std::to_string(idx + 4), c.latent_channels * c.num_latents, c.int_channels, 3, c.int_channels,
             &v->enc[k++]));
  // ---- decoder (vae.py:123-172) ----
  TRY(b.conv("decoder.0", c.int_channels, c.latent_channels, 3, bke(dt), &v->dec_in));
  idx = 2;
  int cin = c.int_channels;
  for (int i = 0; i < c.num_upscalers; ++i) {
    ConvW& t = v->convt[i];
    const int Co = c.upscale_channels;
    const float *w, *bias;
    TRY(wm.get("decoder." + std::to_string(idx) + ".weight", (int64_t)cin * Co * 4, &w));
    TRY(wm.get("decoder." + std::to_string(idx) + ".bias", Co, &bias));
    t.N = 4 * Co; t.n_valid = 4 * Co; t.cin_pad = cin; t.taps = 1; t.cout = Co;
    TRY(v->arena.alloc(&t.w, (size_t)4 * Co * cin * esize(dt)));
    TRY(launch_repack_convt2(w, t.w, cin, Co, dt, s));
    b.weights(t.w, (size_t)4 * Co * cin);
    void* pb;
    TRY(v->arena.alloc(&pb, (size_t)4 * Co * sizeof(float)));
    for (int q = 0; q < 4; ++q)
      HIP_TRY(hipMemcpyAsync((float*)pb + q * Co, bias, Co * sizeof(float), hipMemcpyDeviceToDevice, s));
    t.bias = (float*)pb;
    b.nparams += (int64_t)cin * Co * 4 + Co;
    TRY(b.norm("decoder." + std::to_string(idx + 1), Co, &v->ln[i]));
    cin = Co;
    idx += 3;
  }
  TRY(b.norm("decoder." + std::to_string(idx), cin, &v->dec_gn));
  TRY(b.conv("decoder." + std::to_string(idx + 2), c.out_channels, cin, 3, cin, &v->dec_out));
  if (dt == DT_F32) {
    // the data-gradient packings (the planes of a bf16x3 handle are made by vae_pack_decoder itself: not registered with b.weights)
    dgrad_conv_shape(&v->dec_in_d, c.int_channels, c.latent_channels, EPI_NCHW_F32);
    dgrad_conv_shape(&v->dec_out_d, c.out_channels, cin, EPI_STORE);
    TRY(v->arena.alloc(&v->dec_in_d.w, convw_floats(v->dec_in_d) * sizeof(float)));
    TRY(v->arena.alloc(&v->dec_out_d.w, convw_floats(v->dec_out_d) * sizeof(float)));
    int ci = c.int_channels;
    for (int i = 0; i < c.num_upscalers; ++i) {
      dgrad_convt_shape(&v->convt_d[i], ci, c.upscale_channels);
      TRY(v->arena.alloc(&v->convt_d[i].w, convw_floats(v->convt_d[i]) * sizeof(float)));
      ci = c.upscale_channels;
    }
    TRY(vae_pack_decoder(v, wm, s, false));
    if (encoder_backward_ok(c)) {
      const std::vector<EncLayer> l = encoder_layers(c);
      for (int i = 1; i < kEncLayers; ++i) {
        if (l[i].stride == 2) dgrad_conv_s2_shape(&v->enc_d[i], l[i].Co, l[i].Ci);
        else dgrad_conv_shape(&v->enc_d[i], l[i].Co, l[i].Ci, EPI_STORE);
        TRY(v->arena.alloc(&v->enc_d[i].w, convw_floats(v->enc_d[i]) * sizeof(float)));
      }
      TRY(vae_pack_encoder(v, wm, s, false));
    }
  }
  return b.finish(*v);
}

struct ArgmaxOut { int64_t* ids = nullptr; float* prob = nullptr; float mask_th = -1.f; int64_t ignore_label = 0; };
// fused evaluation tail (ldmseg_vae_decode_panoptic): host-side per-image geometry + device outputs
struct PanopticOut {
  int in_h = 0, in_w = 0;
  const int32_t* boxes = nullptr; const int32_t* sizes = nullptr; const int64_t* offsets = nullptr;
  int threshold_output = 0, threshold_mode = 0;
  float mask_th = 0.5f; int count_th = 0; double overlap_th = 0.0; int64_t ignore_label = 0;
  int32_t* labels = nullptr; int32_t* panoptic = nullptr; uint8_t* keep = nullptr; int32_t* counts = nullptr; int32_t* mask_counts = nullptr;
  int mask_rule = 0;       // overlap mask: 0 sigmoid(logit) >= mask_th (trainers_ldm_cond.py:1288,1301), 1 logit >= mask_th (trainers_ae.py:656)
};
// fused mIoU tail (ldmseg_vae_decode_semseg / ldmseg_vae_reconstruct_semseg): trainers_ae.py:754-761 + SemsegMeter.update
struct SemsegOut {
  int out_h = 0, out_w = 0;
  float mask_th = -1.f; int64_t ignore_label = 0;
  const int64_t* targets = nullptr; int64_t ignore_index = 255; int K = 0;
  int64_t* preds = nullptr; int64_t* counts = nullptr;
};

// What becomes of the decoder's logits: fp32 NCHW at 4L straight from the last conv | bilinear x2 -> fp32 NCHW | x2 + argmax + max-softmax |
// resampling + panoptic post-processing | align_corners=True resampling + argmax / threshold + meter counters; and that tail's outputs
struct DecodeTail {
  enum Kind { LOGITS, LOGITS_X2, ARGMAX, PANOPTIC, SEMSEG } kind = LOGITS;
  float* logits = nullptr;
  const ArgmaxOut* am = nullptr;
  const PanopticOut* po = nullptr;
  const SemsegOut* so = nullptr;
};

// the decoder on an executor that is already set up (the reconstruct chain runs encoder and decoder on ONE workspace pass)
int vae_decode_body(Exec& ex, ldmseg_vae* v, const float* z, float z_scale, int L, const DecodeTail& tail) {
  const int B = ex.B;
  hipStream_t s = ex.s;
  const int dt = v->dt;
  const ldmseg_vae_cfg& c = v->cfg;
  Act zin = ex.new_act(bke(dt), L, L, true);
  TRY(ex.launch("launch_pack_nchw failed", 4, 0, 0, no_label, [&] { return launch_pack_nchw(z, zin.p, B, c.latent_channels, L * L, bke(dt), z_scale, 0.f, dt, s); }));
  Act h;
  TRY(ex.conv(v->dec_in, zin, &h));
  for (int i = 0; i < c.num_upscalers; ++i) {
    const ConvW& t = v->convt[i];
    Act o = ex.new_act(t.cout, 2 * h.H, 2 * h.W, true);
    IgemmParams p;
    p.src0 = h.p; p.C0 = h.C; p.B = B; p.Hi = p.Ho = h.H; p.Wi = p.Wo = h.W;
    p.M = B * h.H * h.W; p.N = t.N; p.n_valid = t.N; p.W = t.w; p.bias = t.bias;
    p.out = o.p; p.ldo = t.cout; p.epi = EPI_CONVT2; p.cout = t.cout;
    TRY(ex.igemm(p));
    Act n;
    TRY(ex.layernorm(v->ln[i], o, 1e-6f, 1, &n, true));   // LayerNorm2d + SiLU, in place
    h = n;
  }
  Act g;
  TRY(ex.groupnorm(v->dec_gn, h, nullptr, 1e-5f, 1, &g));
  const int H4 = h.H, W4 = h.W, Co = c.out_channels;
  IgemmParams p;
  p.src0 = g.p; p.C0 = g.C; p.B = B; p.Hi = p.Ho = H4; p.Wi = p.Wo = W4;
  p.taps = 9; p.M = B * H4 * W4; p.N = v->dec_out.N; p.n_valid = Co;
  p.W = v->dec_out.w; p.bias = v->dec_out.bias;
  if (tail.kind == DecodeTail::LOGITS) {
    p.out = tail.logits; p.epi = EPI_NCHW_F32;
    TRY(ex.igemm(p));
    return 0;
  }
  // every other tail reads NHWC logits at 4L
  Act lo = ex.new_act(Co, H4, W4, false);
  p.out = lo.p; p.ldo = Co; p.epi = EPI_STORE;
  TRY(ex.igemm(p));
  const double lo_bytes = (double)B * H4 * W4 * Co * esize(dt);
  if (tail.kind == DecodeTail::PANOPTIC) {
    const PanopticOut* po = tail.po;
    return ex.launch("launch_panoptic_from_decoder failed", 4, 0, lo_bytes, no_label, [&] {
      return launch_panoptic_from_decoder(lo.p, B, H4, W4, Co, dt, po->in_h, po->in_w, po->boxes, po->sizes, po->offsets, po->threshold_output,
                                          po->threshold_mode, po->mask_th, po->count_th, po->overlap_th, po->ignore_label, po->labels,
                                          po->panoptic, po->keep, po->counts, po->mask_counts, s, nullptr, po->mask_rule);
    }, "decode_panoptic: bad crop box / output size / class count");
  }
  if (tail.kind == DecodeTail::SEMSEG) {
    const SemsegOut* so = tail.so;
    return ex.launch("launch_semseg_from_decoder failed", 4, 0, lo_bytes + (double)B * so->out_h * so->out_w * 16.0,
                     [&] { return "semseg_tail " + std::to_string(so->out_h) + "x" + std::to_string(so->out_w); }, [&] {
      return launch_semseg_from_decoder(lo.p, B, H4, W4, Co, dt, so->out_h, so->out_w, so->mask_th, so->ignore_label, so->targets,
                                        so->ignore_index, so->K, so->preds, so->counts, s);
    }, "decode_semseg: bad output size / class count");
  }
  if (const ArgmaxOut* am = tail.kind == DecodeTail::ARGMAX ? tail.am : nullptr)
    return ex.launch("launch_bilinear2x_argmax failed", 4, 0, lo_bytes + (double)B * 4 * H4 * W4 * 12.0, no_label,
                     [&] { return launch_bilinear2x_argmax(lo.p, am->ids, am->prob, B, H4, W4, Co, am->mask_th, am->ignore_label, dt, s); });
  return ex.launch("launch_bilinear2x_nchw failed", 4, 0, (double)B * H4 * W4 * Co * (esize(dt) + 16.0), no_label,
                   [&] { return launch_bilinear2x_nchw(lo.p, tail.logits, B, H4, W4, Co, dt, s); });
}

// a decode as a planned pass of its own
int vae_decode(ldmseg_vae* v, const float* z, float z_scale, int B, int L, const DecodeTail& tail, void* stream) {
  return plan_and_run(*v, nullptr, [&](bool dry, size_t scratch_base) {
    Exec ex = make_exec(*v, B, (hipStream_t)stream, dry, scratch_base);
    return vae_decode_body(ex, v, z, z_scale, L, tail);
  });
}

// ---- the decoder's backward.  One planned pass: the decoder forward again up to the GroupNorm output (the logits
// themselves are not needed), keeping what the backward reads, then the chain from d loss / d logits down to every parameter
// gradient asked for (g[slot], slots as decoder_keys; null = skipped) and to grad_z.
struct WgradJob {
  const float* dy; int ldy, N;        // dY [P][ldy], N columns taken
  const float* x; int C;              // X [P][C]
  int H, W, taps, form, n_real, c_real, co;      // H x W: the map X lives on
  int stride = 1; WgradRule rule = kWgradFixedTile;   // the encoder's launches (WgradParams)
};
int run_wgrad(Exec& ex, const WgradJob& j, float* out) {
  if (!out) return 0;
  Workspace* ws = ex.ws;
  const size_t m = ws->mark();
  WgradParams wp;
  wp.dy = j.dy; wp.ldy = j.ldy; wp.x = j.x; wp.B = ex.B; wp.H = j.H; wp.W = j.W; wp.N = j.N; wp.C = j.C; wp.taps = j.taps;
  wp.x3 = ex.x3 ? 1 : 0; wp.stride = j.stride; wp.rule = j.rule;
  WgradPlan pl;
  if (wgrad_plan(wp, wgrad_cus(), &pl)) return fail(LDMSEG_E_SHAPE, "weight gradient: unsupported shape");
  wp.partial = (float*)ws->scratch(wgrad_partial_bytes(wp, pl));
  const double P = (double)ex.B * conv_out_dim(j.H, j.stride) * conv_out_dim(j.W, j.stride);
  const int r = ex.launch("launch_wgrad failed", 0, 2.0 * P * j.n_real * j.c_real * j.taps, P * (j.N + j.C) * 4.0 * pl.tiles / pl.n_tiles,
                          [&] {      // (no commas: the profile dump is a CSV)
                            return std::string(pl.x3 ? "wgrad x3" : "wgrad f32") + " P=" + std::to_string((long long)P) + " N=" + std::to_string(j.N) +
                                   " C=" + std::to_string(j.C) + " taps=" + std::to_string(j.taps) + " slices=" + std::to_string(pl.slices) +
                                   " grid=" + std::to_string(pl.grid_x) +
                                   (j.rule == kWgradByWidth ? " tile=" + std::to_string(pl.tile_n) + "x" + std::to_string(pl.tile_c) + " stride=" + std::to_string(j.stride) : std::string());
                          }, [&] { return launch_wgrad(wp, pl, {j.form, j.n_real, j.c_real, j.co, out}, ex.s); });
  ws->reset(m);
  return r;
}
int run_colsum(Exec& ex, const float* a, int lda, int P, int Q, int qstride, int n, float* out) {
  if (!out) return 0;
  Workspace* ws = ex.ws;
  const size_t m = ws->mark();
  float* scratch = (float*)ws->scratch(colsum_scratch_bytes(P, lda));
  const int r = ex.launch("launch_colsum failed", 4, 0, (double)P * lda * 4.0, [&] { return "colsum P=" + std::to_string(P) + " N=" + std::to_string(lda); },
                          [&] { return launch_colsum(a, lda, P, lda, Q, qstride, n, scratch, out, ex.s); });
  ws->reset(m);
  return r;
}

int vae_decode_backward_body(Exec& ex, ldmseg_vae* v, const float* z, float z_scale, int L, const float* grad_logits, float* grad_z,
                             float* const* g) {
  const int B = ex.B;
  hipStream_t s = ex.s;
  const int dt = v->dt;
  const ldmseg_vae_cfg& c = v->cfg;
  const int U = c.num_upscalers, Cu = c.upscale_channels, Co = c.out_channels;
  // ---- forward again, everything the backward reads is kept
  Act zin = ex.new_act(bke(dt), L, L, true);
  TRY(ex.launch("launch_pack_nchw failed", 4, 0, 0, no_label, [&] { return launch_pack_nchw(z, zin.p, B, c.latent_channels, L * L, bke(dt), z_scale, 0.f, dt, s); }));
  Act h;
  TRY(ex.conv(v->dec_in, zin, &h));
  Act hin[4], pre[4];
  for (int i = 0; i < U; ++i) {
    const ConvW& t = v->convt[i];
    hin[i] = h;
    pre[i] = ex.new_act(t.cout, 2 * h.H, 2 * h.W, true);
    IgemmParams p;
    p.src0 = h.p; p.C0 = h.C; p.B = B; p.Hi = p.Ho = h.H; p.Wi = p.Wo = h.W;
    p.M = B * h.H * h.W; p.N = t.N; p.n_valid = t.N; p.W = t.w; p.bias = t.bias;
    p.out = pre[i].p; p.ldo = t.cout; p.epi = EPI_CONVT2; p.cout = t.cout;
    TRY(ex.igemm(p));
    Act n;
    TRY(ex.layernorm(v->ln[i], pre[i], 1e-6f, 1, &n, false));   // out of place: the transposed conv's own output is the backward's input
    h = n;
  }
  Act gact;
  TRY(ex.groupnorm(v->dec_gn, h, nullptr, 1e-5f, 1, &gact));
  // ---- backward
  Workspace* ws = ex.ws;
  const int H4 = h.H, W4 = h.W, P4 = B * H4 * W4;
  const int Cop = (int)rup(Co, bke(dt));
  const size_t last = (size_t)2 + 4 * U;          // slot of the GroupNorm weight
  float* dyp = (float*)ws->scratch((size_t)P4 * Cop * sizeof(float));
  TRY(ex.launch("launch_pack_nchw failed", 4, 0, 0, [] { return std::string("pack grad_logits"); }, [&] { return launch_pack_nchw(grad_logits, dyp, B, Co, H4 * W4, Cop, 1.f, 0.f, dt, s); }));
  TRY(run_wgrad(ex, {dyp, Cop, Cop, (const float*)gact.p, Cu, H4, W4, 9, 0, Co, Cu, 0}, g[last + 2]));
  TRY(run_colsum(ex, dyp, Cop, P4, 1, 0, Co, g[last + 3]));
  Act dg = ex.new_act(Cu, H4, W4, false);
  {
    IgemmParams p;
    p.src0 = dyp; p.C0 = Cop; p.B = B; p.Hi = p.Ho = H4; p.Wi = p.Wo = W4;
    p.taps = 9; p.M = P4; p.N = v->dec_out_d.N; p.n_valid = Cu; p.W = v->dec_out_d.w;
    p.out = dg.p; p.ldo = Cu; p.epi = EPI_STORE;
    TRY(ex.igemm(p));
  }
  Act dh = ex.new_act(Cu, H4, W4, false);
  {
    float* scratch = (float*)ws->scratch(gn_bwd_scratch_bytes(B, Cu));
    TRY(ex.launch("launch_gn_silu_bwd failed", 2, 0, 4.0 * P4 * Cu * 4.0, [&] { return "gn_silu_bwd HW=" + std::to_string(H4 * W4) + " C=" + std::to_string(Cu); }, [&] {
      return launch_gn_silu_bwd((const float*)h.p, (const float*)dg.p, v->dec_gn.g, v->dec_gn.b, (float*)dh.p, g[last], g[last + 1], B, H4 * W4, Cu,
                                1e-5f, scratch, s);
    }));
  }
  for (int i = U - 1; i >= 0; --i) {
    const size_t slot = (size_t)2 + 4 * i;
    const Act& x = hin[i];                         // the transposed conv's input, on the low-resolution map
    const int Pl = B * x.H * x.W, M = 4 * Pl;
    // LayerNorm2d + SiLU backward; its result is stored phase-major [B, H, W, 2x2, Cu]: both transposed-conv gradients read it as
    // a [Pl][4 Cu] matrix without a repack
    Act dpre = ex.new_act(Cu, pre[i].H, pre[i].W, false);
    {
      float* scratch = (float*)ws->scratch(ln_bwd_scratch_bytes(M, Cu));
      TRY(ex.launch("launch_ln_silu_bwd failed", 3, 0, 3.0 * M * Cu * 4.0, [&] { return "ln_silu_bwd M=" + std::to_string(M) + " C=" + std::to_string(Cu); }, [&] {
        return launch_ln_silu_bwd((const float*)pre[i].p, (const float*)dh.p, v->ln[i].g, v->ln[i].b, (float*)dpre.p, g[slot + 2], g[slot + 3], M, Cu,
                                  1e-6f, 1, pre[i].H, pre[i].W, scratch, s);
      }));
    }
    TRY(run_wgrad(ex, {(const float*)dpre.p, 4 * Cu, 4 * Cu, (const float*)x.p, x.C, x.H, x.W, 1, 1, 4 * Cu, x.C, Cu}, g[slot]));
    TRY(run_colsum(ex, (const float*)dpre.p, 4 * Cu, Pl, 4, Cu, Cu, g[slot + 1]));
    Act dx = ex.new_act(x.C, x.H, x.W, false);
    IgemmParams p;
    p.src0 = dpre.p; p.C0 = 4 * Cu; p.B = B; p.Hi = p.Ho = x.H; p.Wi = p.Wo = x.W;
    p.taps = 1; p.M = Pl; p.N = v->convt_d[i].N; p.n_valid = x.C; p.W = v->convt_d[i].w;
    p.out = dx.p; p.ldo = x.C; p.epi = EPI_STORE;
    TRY(ex.igemm(p));
    dh = dx;
  }
  const int P0 = B * L * L, Ci = c.int_channels;
  TRY(run_wgrad(ex, {(const float*)dh.p, Ci, Ci, (const float*)zin.p, zin.C, L, L, 9, 0, Ci, c.latent_channels, 0}, g[0]));
  TRY(run_colsum(ex, (const float*)dh.p, Ci, P0, 1, 0, Ci, g[1]));
  if (grad_z) {
    IgemmParams p;
    p.src0 = dh.p; p.C0 = Ci; p.B = B; p.Hi = p.Ho = L; p.Wi = p.Wo = L;
    p.taps = 9; p.M = P0; p.N = v->dec_in_d.N; p.n_valid = c.latent_channels; p.W = v->dec_in_d.w;
    p.out = grad_z; p.epi = EPI_NCHW_F32;
    TRY(ex.igemm(p));
    if (z_scale != 1.0f)     // decode(z, z_scale) feeds z * z_scale
      TRY(ex.launch("launch_axpby failed", 4, 0, 0, no_label, [&] { return launch_axpby(grad_z, z_scale, 0.f, grad_z, (size_t)P0 * c.latent_channels, s); }));
  }
  return 0;
}

// ---- the encoder's backward.  One planned pass: the encoder forward again up to the GroupNorm output (the moments
// themselves are not needed), the four conv + SiLU layers as a SiLU-less conv that keeps the pre-activation u plus one silu_fwd
// launch, then the chain from d loss / d moments down to every parameter gradient asked for (g[slot], slots as encoder_keys; null =
// skipped).  The chain stops below the lowest layer a gradient is asked of; the input is data.
int vae_encode_backward_body(Exec& ex, ldmseg_vae* v, const float* x, float mul, float add, int H, const float* grad_moments, float* const* g) {
  const int B = ex.B;
  hipStream_t s = ex.s;
  const int dt = v->dt;
  const ldmseg_vae_cfg& c = v->cfg;
  const std::vector<EncLayer> l = encoder_layers(c);
  const int last = kEncLayers - 1;
  // the lowest layer whose parameters are asked for (the GroupNorm sits between layers 7 and 8)
  int lowest = kEncLayers;
  for (int k = last; k >= 0; --k)
    if (g[enc_slot(k)] || g[enc_slot(k) + 1]) lowest = k;
  if ((g[kEncNormSlot] || g[kEncNormSlot + 1]) && lowest > last) lowest = last;
  if (lowest == kEncLayers) return 0;
  // ---- forward again, everything the backward reads is kept: in[k] = the input of layer k, u[k] = the pre-activation of a SiLU layer
  Act in[kEncLayers], u[kEncLayers];
  in[0] = ex.new_act(bke(dt), H, H, true);
  TRY(ex.launch("launch_pack_nchw failed", 4, 0, 0, no_label, [&] { return launch_pack_nchw(x, in[0].p, B, c.in_channels, H * H, bke(dt), mul, add, dt, s); }));
  Act h7;
  for (int k = 0; k < last; ++k) {
    Act o;
    TRY(ex.conv(v->enc[k], in[k], &o, {.stride = l[k].stride}));
    if (l[k].silu) {
      u[k] = o;
      Act a = ex.new_act(o.C, o.H, o.W, true);
      const size_t n = (size_t)B * o.H * o.W * o.C;
      TRY(ex.launch("launch_silu_fwd failed", 4, 0, 8.0 * n, no_label, [&] { return launch_silu_fwd((const float*)o.p, (float*)a.p, n, s); }));
      o = a;
    }
    if (k + 1 < last) in[k + 1] = o; else h7 = o;
  }
  TRY(ex.groupnorm(v->enc_gn, h7, nullptr, 1e-6f, 1, &in[last]));
  // ---- backward: the running gradient alternates between two buffers of the largest activation's size
  Workspace* ws = ex.ws;
  const int l8 = h7.H, P8 = B * l8 * l8, Cm = (int)rup(l[last].Co, bke(dt)), Ci8 = c.int_channels;
  size_t gmax = (size_t)P8 * Ci8;
  for (int k = 1; k < last; ++k) gmax = std::max(gmax, (size_t)B * in[k].H * in[k].W * in[k].C);
  float* gb[2] = {(float*)ws->scratch(gmax * sizeof(float)), (float*)ws->scratch(gmax * sizeof(float))};
  float* dm = (float*)ws->scratch((size_t)P8 * Cm * sizeof(float));
  TRY(ex.launch("launch_pack_nchw failed", 4, 0, 0, [] { return std::string("pack grad_moments"); }, [&] { return launch_pack_nchw(grad_moments, dm, B, l[last].Co, l8 * l8, Cm, 1.f, 0.f, dt, s); }));
  TRY(run_wgrad(ex, {dm, Cm, Cm, (const float*)in[last].p, Ci8, l8, l8, 9, 0, l[last].Co, Ci8, 0, 1, kWgradByWidth}, g[kEncHeadSlot]));
  TRY(run_colsum(ex, dm, Cm, P8, 1, 0, l[last].Co, g[kEncHeadSlot + 1]));
  if (lowest == last && !g[kEncNormSlot] && !g[kEncNormSlot + 1]) return 0;
  {
    IgemmParams p;
    p.src0 = dm; p.C0 = Cm; p.B = B; p.Hi = p.Ho = l8; p.Wi = p.Wo = l8;
    p.taps = 9; p.M = P8; p.N = v->enc_d[last].N; p.n_valid = Ci8; p.W = v->enc_d[last].w;
    p.out = gb[0]; p.ldo = Ci8; p.epi = EPI_STORE;
    TRY(ex.igemm(p));
  }
  {
    const size_t m = ws->mark();
    float* scratch = (float*)ws->scratch(gn_bwd_scratch_bytes(B, Ci8));
    TRY(ex.launch("launch_gn_silu_bwd failed", 2, 0, 4.0 * P8 * Ci8 * 4.0, [&] { return "gn_silu_bwd HW=" + std::to_string(l8 * l8) + " C=" + std::to_string(Ci8); }, [&] {
      return launch_gn_silu_bwd((const float*)h7.p, gb[0], v->enc_gn.g, v->enc_gn.b, gb[1], g[kEncNormSlot], g[kEncNormSlot + 1], B, l8 * l8, Ci8, 1e-6f,
                                scratch, s);
    }));
    ws->reset(m);
  }
  int cur = 1;                                   // gb[cur] = d loss / d (output of layer k before its SiLU)
  for (int k = last - 1; k >= lowest; --k) {
    const Act& xi = in[k];                       // the layer's input, on the map H x W of X
    const int Co = l[k].Co, st = l[k].stride;
    const int Ho = conv_out_dim(xi.H, st), Wo = conv_out_dim(xi.W, st), Po = B * Ho * Wo;
    TRY(run_wgrad(ex, {gb[cur], Co, Co, (const float*)xi.p, xi.C, xi.H, xi.W, 9, 0, Co, l[k].Ci, 0, st, kWgradByWidth}, g[enc_slot(k)]));
    TRY(run_colsum(ex, gb[cur], Co, Po, 1, 0, Co, g[enc_slot(k) + 1]));
    if (k == lowest) break;
    const ConvW& d = v->enc_d[k];
    IgemmParams p;
    p.src0 = gb[cur]; p.C0 = Co; p.B = B; p.Hi = p.Ho = Ho; p.Wi = p.Wo = Wo;
    p.taps = 9; p.M = Po; p.N = d.N; p.W = d.w; p.out = gb[1 - cur]; p.ldo = xi.C;
    if (st == 2) { p.n_valid = 4 * xi.C; p.epi = EPI_CONVT2; p.cout = xi.C; }
    else { p.n_valid = xi.C; p.epi = EPI_STORE; }
    TRY(ex.igemm(p));
    cur = 1 - cur;
    if (l[k - 1].silu) {                         // the input was SiLU(u[k - 1]): in place
      const size_t n = (size_t)B * xi.H * xi.W * xi.C;
      TRY(ex.launch("launch_silu_bwd failed", 4, 0, 12.0 * n, no_label, [&] { return launch_silu_bwd((const float*)u[k - 1].p, gb[cur], gb[cur], n, s); }));
    }
  }
  return 0;
}

int vae_encode_body(Exec& ex, ldmseg_vae* v, const float* x, float mul, float add, int H, float* moments) {
  const int B = ex.B;
  hipStream_t s = ex.s;
  const int dt = v->dt;
  const ldmseg_vae_cfg& c = v->cfg;
  Act xin = ex.new_act(bke(dt), H, H, true);
  TRY(ex.launch("launch_pack_nchw failed", 4, 0, 0, no_label, [&] { return launch_pack_nchw(x, xin.p, B, c.in_channels, H * H, bke(dt), mul, add, dt, s); }));
  Act h, o;
  int k = 0;
  TRY(ex.conv(v->enc[k++], xin, &h, {.silu = 1}));  // conv + SiLU
  for (int i = 0; i < 3; ++i) {
    TRY(ex.conv(v->enc[k++], h, &o)); h = o;
    TRY(ex.conv(v->enc[k++], h, &o, {.stride = 2, .silu = 1})); h = o;
  }
  TRY(ex.conv(v->enc[k++], h, &o)); h = o;
  Act g;
  TRY(ex.groupnorm(v->enc_gn, h, nullptr, 1e-6f, 1, &g));
  const ConvW& last = v->enc[k];
  IgemmParams p;
  p.src0 = g.p; p.C0 = g.C; p.B = B; p.Hi = p.Ho = h.H; p.Wi = p.Wo = h.W;
  p.taps = 9; p.M = B * h.H * h.W; p.N = last.N; p.n_valid = c.latent_channels * c.num_latents;
  p.W = last.w; p.bias = last.bias; p.out = moments; p.epi = EPI_NCHW_F32;
  TRY(ex.igemm(p));
  return 0;
}

// vae_model(images, sample_posterior=False).sample (vae.py:273-307) behind one workspace plan: encode -> posterior mode -> decode
// (interpolate=False, no scaling factor) -> the tail `po` / `so`.  Moments [B,8,l,l] and latents [B,4,l,l] (fp32 NCHW, what
// ldmseg_vae_encode / ldmseg_vae_posterior hand over; the callers refuse latent_channels != 4, which launch_posterior_sample assumes)
// are persistent regions of the handle's workspace.  The plan is the SUM of both halves' persistent activations and the MAXIMUM of
// their scratch peaks: the scratch stack is reset between the halves, which is safe because every launch is on the one stream.
int vae_reconstruct(ldmseg_vae* v, const float* x, float mul, float add, int B, int H, const DecodeTail& tail, void* stream) {
  return plan_and_run(*v, nullptr, [&](bool dry, size_t scratch_base) -> int {
    hipStream_t s = (hipStream_t)stream;
    Exec ex = make_exec(*v, B, s, dry, scratch_base);
    const int l = H / 8;
    float* moments = (float*)v->ws.persist((size_t)B * 8 * l * l * sizeof(float));
    float* z = (float*)v->ws.persist((size_t)B * 4 * l * l * sizeof(float));
    TRY(vae_encode_body(ex, v, x, mul, add, H, moments));
    TRY(ex.launch("launch_posterior_sample failed", 4, 0, 0, no_label, [&] { return launch_posterior_sample(moments, nullptr, z, B, l * l, s); }));
    v->ws.reset(0);      // the decoder reuses the encoder's scratch (same stream: the encoder's launches are ordered before)
    return vae_decode_body(ex, v, z, 1.0f, l, tail);
  });
}

// what the two panoptic entries share: geometry, thresholds and outputs, by name (the caller adds threshold_mode / mask_rule)
PanopticOut panoptic_out(int in_h, int in_w, const int32_t* crop_boxes, const int32_t* out_sizes, const int64_t* out_offsets, int threshold_output,
                         float mask_th, int count_th, double overlap_th, int64_t ignore_label, int32_t* labels, int32_t* panoptic, uint8_t* keep,
                         int32_t* counts, int32_t* mask_counts) {
  return PanopticOut{.in_h = in_h, .in_w = in_w, .boxes = crop_boxes, .sizes = out_sizes, .offsets = out_offsets, .threshold_output = threshold_output,
                     .mask_th = mask_th, .count_th = count_th, .overlap_th = overlap_th, .ignore_label = ignore_label, .labels = labels,
                     .panoptic = panoptic, .keep = keep, .counts = counts, .mask_counts = mask_counts};
}

int semseg_out_check(const ldmseg_vae* h, int out_h, int out_w, const int64_t* targets, int num_classes, const int64_t* counts) {
  if (out_h < 1 || out_w < 1) return fail(LDMSEG_E_SHAPE, "bad output size");
  if (h->cfg.out_channels > 256 || h->cfg.out_channels % 8) return fail(LDMSEG_E_ARG, "the fused tail needs out_channels <= 256, a multiple of 8");
  if (targets && counts && (num_classes < 1 || num_classes > 256)) return fail(LDMSEG_E_ARG, "num_classes must be 1..256");
  return 0;
}

// ------------------------------------------------------------------ image VAE encoder
constexpr int kKLCh[4] = {128, 256, 512, 512};
constexpr int kKLMid = 512;

int klenc_build(ldmseg_vae_image* v, const WeightMap& wm) {
  Builder b(*v, wm);
  hipStream_t s = b.s;
  const int cp = bke(v->dt);
  TRY(b.conv("encoder.conv_in", kKLCh[0], 3, 3, cp, &v->conv_in));
  int cin = kKLCh[0], dummy = 0;
  for (int i = 0; i < 4; ++i) {
    for (int j = 0; j < 2; ++j) {
      TRY(build_resnet(b, "encoder.down_blocks." + std::to_string(i) + ".resnets." + std::to_string(j) + ".", cin, kKLCh[i],
                       &dummy, &v->down[i][j]));
      cin = kKLCh[i];
    }
    if (i < 3) TRY(b.conv("encoder.down_blocks." + std::to_string(i) + ".downsamplers.0.conv", cin, cin, 3, cin, &v->downs[i]));
  }
  for (int j = 0; j < 2; ++j)
    TRY(build_resnet(b, "encoder.mid_block.resnets." + std::to_string(j) + ".", kKLMid, kKLMid, &dummy, &v->mid[j]));
  // single-head attention block; diffusers 0.16.1 names (query/key/value/proj_attn) or the later to_q/.../to_out.0
  const std::string ap = "encoder.mid_block.attentions.0.";
  const bool old_names = wm.m.count(ap + "query.weight") != 0;
  const std::string qn = old_names ? "query" : "to_q", kn = old_names ? "key" : "to_k", vn = old_names ? "value" : "to_v",
                    pn = old_names ? "proj_attn" : "to_out.0";
  TRY(b.norm(ap + "group_norm", kKLMid, &v->attn_gn));
  TRY(b.conv(ap + qn, kKLMid, kKLMid, 1, kKLMid, &v->q));
  TRY(b.conv(ap + kn, kKLMid, kKLMid, 1, kKLMid, &v->k));
  TRY(b.conv(ap + pn, kKLMid, kKLMid, 1, kKLMid, &v->proj));
  {
    const float* w;
    TRY(wm.get(ap + vn + ".weight", (int64_t)kKLMid * kKLMid, &w));
    TRY(b.arena->alloc(&v->wv, (size_t)kKLMid * kKLMid * esize(v->dt)));
    TRY(launch_repack_conv(w, v->wv, kKLMid, kKLMid, 1, 1, kKLMid, kKLMid, v->dt, s));
    b.nparams += (int64_t)kKLMid * kKLMid;
    TRY(b.f32_copy(ap + vn + ".bias", kKLMid, &v->bv));
  }
  TRY(b.norm("encoder.conv_norm_out", kKLMid, &v->norm_out));
  // conv_out writes its 8 channels into a full K tile (zero padded) so that quant_conv (1x1) can consume it
  TRY(b.conv("encoder.conv_out", 8, kKLMid, 3, kKLMid, &v->conv_out, true, cp));
  TRY(b.conv("quant_conv", 8, 8, 1, cp, &v->quant, true, 0, EPI_NCHW_F32));
  return b.finish(*v);
}

// diffusers ResnetBlock2D with temb=None, eps 1e-6 (AutoencoderKL)
int run_resnet_plain(Exec& ex, const ResnetW& r, const Act& x, Act* out) {
  Workspace* ws = ex.ws;
  const size_t m = ws->mark();
  Act n1, h1, n2, sc;
  TRY(ex.groupnorm(r.norm1, x, nullptr, 1e-6f, 1, &n1));
  TRY(ex.conv(r.conv1, n1, &h1, {.persist = false}));
  TRY(ex.groupnorm(r.norm2, h1, nullptr, 1e-6f, 1, &n2));
  const Act* resid = &x;
  if (r.has_shortcut) {
    TRY(ex.conv(r.shortcut, x, &sc, {.persist = false}));
    resid = &sc;
  }
  TRY(ex.conv(r.conv2, n2, out, {.resid = resid}));
  ws->reset(m);
  return 0;
}

// AttentionBlock of the mid block: one head of width C=512 over the N=H*W tokens of each image.  Built from the
// implicit-GEMM kernel: S_b = Q_b K_b^T (fp32 rows) -> row softmax -> V_b^T = W_v X_b^T -> O_b = P_b V_b (+b_v, since
// softmax rows sum to one) -> proj + residual.  Runs once per image, not per denoising step.
int klenc_attention(Exec& ex, const ldmseg_vae_image* v, const Act& x, Act* out) {
  Workspace* ws = ex.ws;
  const size_t m = ws->mark();
  const int C = kKLMid, N = x.H * x.W;
  const size_t es = esize(ex.dt);
  if (N % 64 != 0) return fail(LDMSEG_E_SHAPE, "image VAE attention: (H/8)*(W/8) must be a multiple of 64");
  Act n, q, k, att;
  TRY(ex.groupnorm(v->attn_gn, x, nullptr, 1e-6f, 0, &n));
  TRY(ex.conv(v->q, n, &q, {.persist = false}));
  TRY(ex.conv(v->k, n, &k, {.persist = false}));
  att = ex.new_act(C, x.H, x.W, false);
  float* S = (float*)ws->scratch((size_t)N * N * sizeof(float));
  void* P = ws->scratch((size_t)N * N * es);
  void* Vt = ws->scratch((size_t)C * N * es);
  for (int b = 0; b < ex.B; ++b) {
    const size_t off = (size_t)b * N * C * es;
    {
      IgemmParams p;                                   // S = Q_b K_b^T
      p.src0 = (const char*)q.p + off; p.C0 = C; p.B = 1; p.Hi = p.Ho = N; p.Wi = p.Wo = 1;
      p.M = N; p.N = N; p.n_valid = N; p.W = (const char*)k.p + off; p.out = S; p.ldo = N; p.epi = EPI_ROWS_F32;
      p.w_dynamic = 1;
      TRY(ex.igemm(p));
    }
    TRY(ex.launch("launch_softmax_rows failed", 4, 0, (double)N * N * (4 + es), no_label, [&] { return launch_softmax_rows(S, P, N, N, 1.0f / std::sqrt((float)C), ex.dt, ex.s); }));
    {
      IgemmParams p;                                   // V_b^T [C][N] = W_v X_b^T
      p.src0 = v->wv; p.C0 = C; p.B = 1; p.Hi = p.Ho = C; p.Wi = p.Wo = 1;
      p.M = C; p.N = N; p.n_valid = N; p.W = (const char*)n.p + off; p.out = Vt; p.ldo = N;
      p.w_dynamic = 1;
      TRY(ex.igemm(p));
    }
    {
      IgemmParams p;                                   // O_b = P_b V_b + b_v
      p.src0 = P; p.C0 = N; p.B = 1; p.Hi = p.Ho = N; p.Wi = p.Wo = 1;
      p.M = N; p.N = C; p.n_valid = C; p.W = Vt; p.bias = v->bv; p.out = (char*)att.p + off; p.ldo = C;
      p.w_dynamic = 1;
      TRY(ex.igemm(p));
    }
  }
  TRY(ex.conv(v->proj, att, out, {.resid = &x}));
  ws->reset(m);
  return 0;
}

int klenc_encode_impl(ldmseg_vae_image* v, const float* x, float mul, float add, int B, int H, int W, float* moments,
                      hipStream_t s, bool dry, size_t scratch_base) {
  Exec ex = make_exec(*v, B, s, dry, scratch_base);
  const int dt = v->dt;
  Act xin = ex.new_act(bke(dt), H, W, true);
  TRY(ex.launch("launch_pack_nchw failed", 4, 0, 0, no_label, [&] { return launch_pack_nchw(x, xin.p, B, 3, H * W, bke(dt), mul, add, dt, s); }));
  Act h, o;
  TRY(ex.conv(v->conv_in, xin, &h));
  for (int i = 0; i < 4; ++i) {
    for (int j = 0; j < 2; ++j) { TRY(run_resnet_plain(ex, v->down[i][j], h, &o)); h = o; }
    if (i < 3) { TRY(ex.conv(v->downs[i], h, &o, {.stride = 2, .pad = 0})); h = o; }
  }
  TRY(run_resnet_plain(ex, v->mid[0], h, &o)); h = o;
  TRY(klenc_attention(ex, v, h, &o)); h = o;
  TRY(run_resnet_plain(ex, v->mid[1], h, &o)); h = o;
  Act g, c8;
  TRY(ex.groupnorm(v->norm_out, h, nullptr, 1e-6f, 1, &g));
  TRY(ex.conv(v->conv_out, g, &c8));
  IgemmParams p;
  p.src0 = c8.p; p.C0 = c8.C; p.B = B; p.Hi = p.Ho = h.H; p.Wi = p.Wo = h.W;
  p.taps = 1; p.M = B * h.H * h.W; p.N = v->quant.N; p.n_valid = 8;
  p.W = v->quant.w; p.bias = v->quant.bias; p.out = moments; p.epi = EPI_NCHW_F32;
  TRY(ex.igemm(p));
  return 0;
}

}  // namespace

// =================================================================== C ABI
extern "C" {

int ldmseg_vae_create(const ldmseg_vae_cfg* cfg, int n_weights, const char* const* names, const void* const* dev_ptrs,
                      const int64_t* numels, ldmseg_vae** out) {
  auto check = [](const ldmseg_vae_cfg& c) {
    if (c.num_latents != 2 || c.norm_num_groups != 32) return fail(LDMSEG_E_ARG, "only the gaussian parametrization with 32 groups is supported");
    return 0;
  };
  return create_handle(cfg, n_weights, names, dev_ptrs, numels, check, vae_build, true, out);
}
LDMSEG_HANDLE_ABI(ldmseg_vae)

int ldmseg_vae_decode(ldmseg_vae* h, const float* z, float z_scale, int B, int L, int interpolate, float* logits,
                      void* stream) {
  g_err.clear();
  if (!h || !z || !logits) return fail(LDMSEG_E_ARG, "null argument");
  DeviceGuard dg(h->cfg.device);
  if (B < 1 || L < 1) return fail(LDMSEG_E_SHAPE, "bad B/L");
  const DecodeTail tail{.kind = interpolate ? DecodeTail::LOGITS_X2 : DecodeTail::LOGITS, .logits = logits};
  return vae_decode(h, z, z_scale, B, L, tail, stream);
}

int ldmseg_vae_decode_backward(ldmseg_vae* h, const float* z, float z_scale, int B, int L, const float* grad_logits, float* grad_z, int n,
                               const char* const* names, float* const* grad_ptrs, const int64_t* numels, void* stream) {
  g_err.clear();
  if (!h || !z || !grad_logits) return fail(LDMSEG_E_ARG, "null argument");
  if (n < 0 || (n > 0 && (!names || !grad_ptrs || !numels))) return fail(LDMSEG_E_ARG, "null argument");
  if (h->dt != DT_F32) return fail(LDMSEG_E_ARG, "the decoder backward needs an fp32-storage handle (compute_dtype fp32 or bf16x3), not bf16");
  if (B < 1 || L < 1) return fail(LDMSEG_E_SHAPE, "bad B/L");
  const std::vector<DecKey> keys = decoder_keys(h->cfg);
  std::vector<float*> g(keys.size(), nullptr);
  for (int i = 0; i < n; ++i) {
    const int k = key_slot(keys, names[i], numels[i], "a decoder");
    if (k < 0) return LDMSEG_E_ARG;
    g[k] = grad_ptrs[i];
  }
  DeviceGuard dg(h->cfg.device);
  return plan_and_run(*h, nullptr, [&](bool dry, size_t scratch_base) {
    Exec ex = make_exec(*h, B, (hipStream_t)stream, dry, scratch_base);
    return vae_decode_backward_body(ex, h, z, z_scale, L, grad_logits, grad_z, g.data());
  });
}

int ldmseg_vae_load_decoder(ldmseg_vae* h, int n, const char* const* names, const void* const* dev_ptrs, const int64_t* numels, void* stream) {
  g_err.clear();
  if (!h || n < 0 || (n > 0 && (!names || !dev_ptrs || !numels))) return fail(LDMSEG_E_ARG, "null argument");
  const std::vector<DecKey> keys = decoder_keys(h->cfg);
  WeightMap wm;
  for (int i = 0; i < n; ++i) {
    if (!dev_ptrs[i]) return fail(LDMSEG_E_ARG, "null decoder tensor");
    const int k = key_slot(keys, names[i], numels[i], "a decoder");
    if (k < 0) return LDMSEG_E_ARG;
    wm.m[keys[k].name] = {(const float*)dev_ptrs[i], numels[i]};
  }
  DeviceGuard dg(h->cfg.device);
  return vae_pack_decoder(h, wm, (hipStream_t)stream, true);
}

int ldmseg_vae_decode_argmax(ldmseg_vae* h, const float* z, float z_scale, int B, int L, float mask_th, int64_t ignore_label,
                             int64_t* ids, float* max_prob, void* stream) {
  g_err.clear();
  if (!h || !z || !ids) return fail(LDMSEG_E_ARG, "null argument");
  DeviceGuard dg(h->cfg.device);
  if (B < 1 || L < 1) return fail(LDMSEG_E_SHAPE, "bad B/L");
  if (h->cfg.num_upscalers != 2) return fail(LDMSEG_E_ARG, "the fused tail assumes interpolation_factor 2 (num_upscalers 2)");
  ArgmaxOut am{ids, max_prob, mask_th, ignore_label};
  const DecodeTail tail{.kind = DecodeTail::ARGMAX, .am = &am};
  return vae_decode(h, z, z_scale, B, L, tail, stream);
}

int ldmseg_vae_decode_panoptic(ldmseg_vae* h, const float* z, float z_scale, int B, int L, int in_h, int in_w,
                               const int32_t* crop_boxes, const int32_t* out_sizes, const int64_t* out_offsets,
                               int threshold_output, int threshold_mode, float mask_th, int count_th, double overlap_th,
                               int64_t ignore_label, int32_t* labels, int32_t* panoptic, uint8_t* keep, int32_t* counts,
                               int32_t* mask_counts, void* stream) {
  g_err.clear();
  if (!h || !z || !out_sizes || !out_offsets || !labels || !panoptic || !keep || !counts || !mask_counts)
    return fail(LDMSEG_E_ARG, "null argument");
  if (B < 1 || L < 1 || in_h < 1 || in_w < 1) return fail(LDMSEG_E_SHAPE, "bad B/L/input size");
  if (threshold_mode != 0 && threshold_mode != 1) return fail(LDMSEG_E_ARG, "threshold_mode must be 0 (max) or 1 (topk_diff)");
  if (h->cfg.num_upscalers != 2) return fail(LDMSEG_E_ARG, "the fused tail assumes interpolation_factor 2 (num_upscalers 2)");
  DeviceGuard dg(h->cfg.device);
  PanopticOut po = panoptic_out(in_h, in_w, crop_boxes, out_sizes, out_offsets, threshold_output, mask_th, count_th, overlap_th, ignore_label,
                                labels, panoptic, keep, counts, mask_counts);
  po.threshold_mode = threshold_mode;
  const DecodeTail tail{.kind = DecodeTail::PANOPTIC, .po = &po};
  return vae_decode(h, z, z_scale, B, L, tail, stream);
}

int ldmseg_vae_encode(ldmseg_vae* h, const float* x, float in_mul, float in_add, int B, int H, float* moments,
                      void* stream) {
  g_err.clear();
  if (!h || !x || !moments) return fail(LDMSEG_E_ARG, "null argument");
  DeviceGuard dg(h->cfg.device);
  if (B < 1 || H < 8 || H % 8) return fail(LDMSEG_E_SHAPE, "H must be a multiple of 8");
  return plan_and_run(*h, nullptr, [&](bool dry, size_t scratch_base) {
    Exec ex = make_exec(*h, B, (hipStream_t)stream, dry, scratch_base);
    return vae_encode_body(ex, h, x, in_mul, in_add, H, moments);
  });
}

int ldmseg_vae_encode_backward(ldmseg_vae* h, const float* x, float in_mul, float in_add, int B, int H, const float* grad_moments, int n,
                               const char* const* names, float* const* grad_ptrs, const int64_t* numels, void* stream) {
  g_err.clear();
  if (!h || !x || !grad_moments) return fail(LDMSEG_E_ARG, "null argument");
  if (n < 0 || (n > 0 && (!names || !grad_ptrs || !numels))) return fail(LDMSEG_E_ARG, "null argument");
  if (h->dt != DT_F32) return fail(LDMSEG_E_ARG, "the encoder backward needs an fp32-storage handle (compute_dtype fp32 or bf16x3), not bf16");
  if (!encoder_backward_ok(h->cfg)) return fail(LDMSEG_E_ARG, "the encoder backward needs block_out_channels and int_channels that are multiples of 32");
  if (B < 1 || H < 8 || H % 8) return fail(LDMSEG_E_SHAPE, "H must be a multiple of 8");
  const std::vector<DecKey> keys = encoder_keys(h->cfg);
  std::vector<float*> g(keys.size(), nullptr);
  for (int i = 0; i < n; ++i) {
    const int k = key_slot(keys, names[i], numels[i], "an encoder");
    if (k < 0) return LDMSEG_E_ARG;
    g[k] = grad_ptrs[i];
  }
  DeviceGuard dg(h->cfg.device);
  return plan_and_run(*h, nullptr, [&](bool dry, size_t scratch_base) {
    Exec ex = make_exec(*h, B, (hipStream_t)stream, dry, scratch_base);
    return vae_encode_backward_body(ex, h, x, in_mul, in_add, H, grad_moments, g.data());
  });
}

int ldmseg_vae_load_encoder(ldmseg_vae* h, int n, const char* const* names, const void* const* dev_ptrs, const int64_t* numels, void* stream) {
  g_err.clear();
  if (!h || n < 0 || (n > 0 && (!names || !dev_ptrs || !numels))) return fail(LDMSEG_E_ARG, "null argument");
  const std::vector<DecKey> keys = encoder_keys(h->cfg);
  WeightMap wm;
  for (int i = 0; i < n; ++i) {
    if (!dev_ptrs[i]) return fail(LDMSEG_E_ARG, "null encoder tensor");
    const int k = key_slot(keys, names[i], numels[i], "an encoder");
    if (k < 0) return LDMSEG_E_ARG;
    wm.m[keys[k].name] = {(const float*)dev_ptrs[i], numels[i]};
  }
  DeviceGuard dg(h->cfg.device);
  return vae_pack_encoder(h, wm, (hipStream_t)stream, true);
}

int ldmseg_vae_posterior_backward(const float* moments, const float* noise, float scale, int B, int l, const float* grad_z, float* grad_moments,
                                  void* stream) {
  g_err.clear();
  if (!moments || !grad_z || !grad_moments) return fail(LDMSEG_E_ARG, "null argument");
  if (B < 1 || l < 1) return fail(LDMSEG_E_SHAPE, "bad B/l");
  return launch_code(launch_posterior_backward(moments, noise, scale, grad_z, grad_moments, B, l * l, (hipStream_t)stream), "launch_posterior_backward failed");
}

int ldmseg_vae_decode_semseg(ldmseg_vae* h, const float* z, float z_scale, int B, int L, int out_h, int out_w, float mask_th,
                             int64_t ignore_label, const int64_t* targets, int64_t ignore_index, int num_classes, int64_t* preds,
                             int64_t* counts, void* stream) {
  g_err.clear();
  if (!h || !z) return fail(LDMSEG_E_ARG, "null argument");
  if (B < 1 || L < 1) return fail(LDMSEG_E_SHAPE, "bad B/L");
  TRY(semseg_out_check(h, out_h, out_w, targets, num_classes, counts));
  DeviceGuard dg(h->cfg.device);
  SemsegOut so{out_h, out_w, mask_th, ignore_label, targets, ignore_index, num_classes, preds, counts};
  const DecodeTail tail{.kind = DecodeTail::SEMSEG, .so = &so};
  return vae_decode(h, z, z_scale, B, L, tail, stream);
}

int ldmseg_vae_reconstruct_semseg(ldmseg_vae* h, const float* x, float in_mul, float in_add, int B, int H, int out_h, int out_w,
                                  float mask_th, int64_t ignore_label, const int64_t* targets, int64_t ignore_index,
                                  int num_classes, int64_t* preds, int64_t* counts, void* stream) {
  g_err.clear();
  if (!h || !x) return fail(LDMSEG_E_ARG, "null argument");
  if (B < 1 || H < 8 || H % 8) return fail(LDMSEG_E_SHAPE, "H must be a multiple of 8");
  if (h->cfg.latent_channels != 4) return fail(LDMSEG_E_ARG, "the reconstruct chain assumes 4 latent channels");
  TRY(semseg_out_check(h, out_h, out_w, targets, num_classes, counts));
  DeviceGuard dg(h->cfg.device);
  SemsegOut so{out_h, out_w, mask_th, ignore_label, targets, ignore_index, num_classes, preds, counts};
  const DecodeTail tail{.kind = DecodeTail::SEMSEG, .so = &so};
  return vae_reconstruct(h, x, in_mul, in_add, B, H, tail, stream);
}

int ldmseg_vae_reconstruct_panoptic(ldmseg_vae* h, const float* x, float in_mul, float in_add, int B, int H, int in_h, int in_w,
                                    const int32_t* crop_boxes, const int32_t* out_sizes, const int64_t* out_offsets,
                                    int threshold_output, float mask_th, int count_th, double overlap_th, int64_t ignore_label,
                                    int32_t* labels, int32_t* panoptic, uint8_t* keep, int32_t* counts, int32_t* mask_counts,
                                    void* stream) {
  g_err.clear();
  if (!h || !x || !out_sizes || !out_offsets || !labels || !panoptic || !keep || !counts || !mask_counts)
    return fail(LDMSEG_E_ARG, "null argument");
  if (B < 1 || H < 8 || H % 8 || in_h < 1 || in_w < 1) return fail(LDMSEG_E_SHAPE, "bad B/H/input size");
  if (h->cfg.latent_channels != 4) return fail(LDMSEG_E_ARG, "the reconstruct chain assumes 4 latent channels");
  if (h->cfg.num_upscalers != 2) return fail(LDMSEG_E_ARG, "the fused tail assumes interpolation_factor 2 (num_upscalers 2)");
  DeviceGuard dg(h->cfg.device);
  PanopticOut po = panoptic_out(in_h, in_w, crop_boxes, out_sizes, out_offsets, threshold_output, mask_th, count_th, overlap_th, ignore_label,
                                labels, panoptic, keep, counts, mask_counts);
  po.mask_rule = 1;
  const DecodeTail tail{.kind = DecodeTail::PANOPTIC, .po = &po};
  return vae_reconstruct(h, x, in_mul, in_add, B, H, tail, stream);
}

int ldmseg_vae_image_create(const ldmseg_vae_image_cfg* cfg, int n_weights, const char* const* names,
                            const void* const* dev_ptrs, const int64_t* numels, ldmseg_vae_image** out) {
  return create_handle(cfg, n_weights, names, dev_ptrs, numels, [](const ldmseg_vae_image_cfg&) { return 0; }, klenc_build, true, out);
}
LDMSEG_HANDLE_ABI(ldmseg_vae_image)

int ldmseg_vae_image_encode(ldmseg_vae_image* h, const float* x, float in_mul, float in_add, int B, int H, int W,
                            float* moments, void* stream) {
  g_err.clear();
  if (!h || !x || !moments) return fail(LDMSEG_E_ARG, "null argument");
  DeviceGuard dg(h->cfg.device);
  if (B < 1 || H < 8 || W < 8 || H % 8 || W % 8) return fail(LDMSEG_E_SHAPE, "H and W must be multiples of 8");
  return plan_and_run(*h, nullptr, [&](bool dry, size_t scratch_base) {
    return klenc_encode_impl(h, x, in_mul, in_add, B, H, W, moments, (hipStream_t)stream, dry, scratch_base);
  });
}

}  // extern "C"
