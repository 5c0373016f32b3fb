// The two VAEs of libldmseg_hip.so with their C ABI (include/ldmseg_hip.h): the seg-VAE (encoder, decoder, the fused evaluation
// tails and the reconstruct chain) and the encoder of SD-1.x's image VAE (AutoencoderKL).  The runtime underneath: runtime.h.
#include <cmath>

#include "runtime.h"
#include "vae_bwd.h"

#pragma clang diagnostic ignored "-Wc++20-designator"      // ConvOpt and its like are filled by field name

using namespace ldmseg;
using namespace ldmseg::rt;

// =================================================================== seg-VAE
// One row of a half's layer table (encoder_rows / decoder_rows below: the model's layers in order) and what the handle holds for
// it.  Row i's reference keys are prefix.weight and prefix.bias: slots 2 i and 2 i + 1 of the name lists the ABI takes.
enum RowKind { ROW_CONV3, ROW_CONVT2, ROW_LN, ROW_GN };     // Conv2d 3x3 pad 1 | ConvTranspose2d k2 s2 | LayerNorm2d | GroupNorm
struct VaeRow {
  RowKind kind;
  std::string prefix;
  int Co, Ci;              // (a norm row: both its channel count)
  int stride, silu;        // silu: SiLU follows - in the conv's epilogue, inside the norm's launch
  int cin_pad, n_store;    // storage widths of a conv: the input's channels as stored, the output channels stored (0: Co)
  int dgrad_epi;           // the epilogue of the row's data-gradient GEMM, -1: the handle packs none (bf16 storage, or the input is data)
  float eps;               // norm rows
};
struct RowW { ConvW w, d; NormW n; };       // forward packing, data-gradient packing (ldmseg_vae_*_backward), norm vectors
struct VaeHalf { std::vector<VaeRow> rows; std::vector<RowW> w; };       // w[i] belongs to rows[i]; the last row is the head conv
struct ldmseg_vae : HandleBase {
  ldmseg_vae_cfg cfg{};
  VaeHalf enc, dec;
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
size_t convw_floats(const ConvW& d) { return (size_t)d.N * d.taps * d.cin_pad; }

// the encoder's backward needs every activation width to be its channel count (no padded channels between the layers)
bool encoder_backward_ok(const ldmseg_vae_cfg& c) {
  for (int i = 0; i < 4; ++i)
    if (c.block_out_channels[i] % 32) return false;
  return c.int_channels % 32 == 0 && c.latent_channels * c.num_latents <= 32;
}

// ---- the two layer tables, pure functions of the configuration.  Everything that walks a half - build, (re)pack, the forward,
// the backward, the ABI's name lists - reads these rows; the state-dict indices appear nowhere else.
// encoder (vae.py:174-244): conv+SiLU, [conv, stride-2 conv+SiLU] x 3, conv, GroupNorm+SiLU, conv
std::vector<VaeRow> encoder_rows(const ldmseg_vae_cfg& c) {
  const int dt = c.compute_dtype == LDMSEG_BF16 ? DT_BF16 : DT_F32;
  const bool dgrad = dt == DT_F32 && encoder_backward_ok(c);
  const int* boc = c.block_out_channels;
  std::vector<VaeRow> r;
  auto conv = [&](int idx, int Co, int Ci, int stride, int silu, int cin_pad, int n_store) {
    const int epi = (!dgrad || idx == 0) ? -1 : stride == 2 ? EPI_CONVT2 : EPI_STORE;      // (the first conv's input is data)
    r.push_back({ROW_CONV3, "encoder." + std::to_string(idx), Co, Ci, stride, silu, cin_pad, n_store, epi, 0.f});
  };
  conv(0, boc[0], c.in_channels, 1, 1, bke(dt), cstore(boc[0], dt));
  int idx = 2;
  for (int i = 0; i < 3; ++i) {
    conv(idx, boc[i], boc[i], 1, 0, cstore(boc[i], dt), cstore(boc[i], dt));
    conv(idx + 1, boc[i + 1], boc[i], 2, 1, cstore(boc[i], dt), cstore(boc[i + 1], dt));
    idx += 3;
  }
  conv(idx, c.int_channels, boc[3], 1, 0, cstore(boc[3], dt), 0);
  r.push_back({ROW_GN, "encoder." + std::to_string(idx + 2), c.int_channels, c.int_channels, 1, 1, 0, 0, -1, 1e-6f});
  conv(idx + 4, c.latent_channels * c.num_latents, c.int_channels, 1, 0, c.int_channels, 0);
  return r;
}
// decoder (vae.py:123-172): conv, [ConvTranspose2d, LayerNorm2d+SiLU] x num_upscalers, GroupNorm+SiLU, conv
std::vector<VaeRow> decoder_rows(const ldmseg_vae_cfg& c) {
  const int dt = c.compute_dtype == LDMSEG_BF16 ? DT_BF16 : DT_F32;
  std::vector<VaeRow> r;
  auto row = [&](RowKind kind, int idx, int Co, int Ci, int stride, int cin_pad, int dgrad_epi, float eps) {
    const bool norm = kind == ROW_LN || kind == ROW_GN;
    r.push_back({kind, "decoder." + std::to_string(idx), Co, Ci, stride, norm, cin_pad, 0, (norm || dt != DT_F32) ? -1 : dgrad_epi, eps});
  };
  row(ROW_CONV3, 0, c.int_channels, c.latent_channels, 1, bke(dt), EPI_NCHW_F32, 0.f);      // (its data gradient is grad_z)
  int idx = 2, cin = c.int_channels;
  for (int i = 0; i < c.num_upscalers; ++i) {
    row(ROW_CONVT2, idx, c.upscale_channels, cin, 2, cin, EPI_STORE, 0.f);
    row(ROW_LN, idx + 1, c.upscale_channels, c.upscale_channels, 1, 0, -1, 1e-6f);
    cin = c.upscale_channels;
    idx += 3;
  }
  row(ROW_GN, idx, cin, cin, 1, 0, -1, 1e-5f);
  row(ROW_CONV3, idx + 2, c.out_channels, cin, 1, cin, EPI_STORE, 0.f);
  return r;
}

// reference keys of a half in model order with their element counts: (weight, bias) of every row
struct VaeKey { std::string name; int64_t numel; };
int64_t weight_numel(const VaeRow& r) {
  return r.kind == ROW_CONV3 ? (int64_t)r.Co * r.Ci * 9 : r.kind == ROW_CONVT2 ? (int64_t)r.Ci * r.Co * 4 : r.Co;
}
std::vector<VaeKey> row_keys(const std::vector<VaeRow>& rows) {
  std::vector<VaeKey> k;
  for (const VaeRow& r : rows) {
    k.push_back({r.prefix + ".weight", weight_numel(r)});
    k.push_back({r.prefix + ".bias", r.Co});
  }
  return k;
}

// name -> slot of `keys`, with the checks the backward and the load entries share; -1 and the message set on a bad name or numel
int key_slot(const std::vector<VaeKey>& keys, const char* name, int64_t numel, const char* what) {
  size_t k = 0;
  while (name && k < keys.size() && keys[k].name != name) ++k;
  if (!name) fail(LDMSEG_E_ARG, "null tensor name");
  else if (k == keys.size()) fail(LDMSEG_E_ARG, std::string("not ") + what + " parameter: " + name);
  else if (numel != keys[k].numel) fail(LDMSEG_E_ARG, keys[k].name + " has " + std::to_string(keys[k].numel) + " elements, got " + std::to_string(numel));
  else return (int)k;
  return -1;
}
// The (n, names, ptrs, numels) of a backward or load entry as pointers by slot (null: a name that was not given).  null_ok: a
// null pointer may come with a name (a gradient that is not wanted).
int by_slot(const std::vector<VaeRow>& rows, bool decoder, int n, const char* const* names, void* const* ptrs, const int64_t* numels, bool null_ok,
            std::vector<void*>* out) {
  const std::vector<VaeKey> keys = row_keys(rows);
  out->assign(keys.size(), nullptr);
  for (int i = 0; i < n; ++i) {
    if (!null_ok && !ptrs[i]) return fail(LDMSEG_E_ARG, decoder ? "null decoder tensor" : "null encoder tensor");
    const int k = key_slot(keys, names[i], numels[i], decoder ? "a decoder" : "an encoder");
    if (k < 0) return LDMSEG_E_ARG;
    (*out)[k] = ptrs[i];
  }
  return 0;
}

// ---- one pack path: a row's source tensors (state-dict layout, fp32, on the device; null: left as it is) into the buffers the
// handle owns - forward packing, data-gradient packing where the row has one, padded bias, norm vectors - for vae_build and
// ldmseg_vae_load_* alike.  A bf16x3 handle's matrices become hi | lo planes right here, once per packing (a second split would
// destroy them: nothing of the seg-VAE is registered with Builder::weights).
int split_x3(const ldmseg_vae* v, const ConvW& m, hipStream_t s) {
  return (v->x3 && v->dt == DT_F32) ? launch_split_planes(m.w, convw_floats(m), s) : 0;
}
int pack_conv3(const ldmseg_vae* v, const VaeRow& r, const RowW& o, const float* w, const float* bias, hipStream_t s) {
  if (w) {
    TRY(launch_repack_conv(w, o.w.w, r.Co, r.Ci, 3, 3, o.w.N, o.w.cin_pad, v->dt, s));
    TRY(split_x3(v, o.w, s));
    if (o.d.w) {
      if (r.stride == 2) TRY(launch_pack_dgrad_conv_s2(w, (float*)o.d.w, r.Co, r.Ci, o.d.N, o.d.cin_pad, s));
      else TRY(launch_pack_dgrad_conv(w, (float*)o.d.w, r.Co, r.Ci, o.d.N, o.d.cin_pad, s));
      TRY(split_x3(v, o.d, s));
    }
  }
  if (bias) TRY(launch_padded_bias(bias, r.Co, o.w.bias, o.w.N, s));
  return 0;
}
int pack_convt2(const ldmseg_vae* v, const VaeRow& r, const RowW& o, const float* w, const float* bias, hipStream_t s) {
  if (w) {
    TRY(launch_repack_convt2(w, o.w.w, r.Ci, r.Co, v->dt, s));
    TRY(split_x3(v, o.w, s));
    if (o.d.w) {
      TRY(launch_pack_dgrad_convt(w, (float*)o.d.w, r.Ci, r.Co, o.d.N, s));
      TRY(split_x3(v, o.d, s));
    }
  }
  if (bias)       // one copy per output phase
    for (int q = 0; q < 4; ++q) HIP_TRY(hipMemcpyAsync(o.w.bias + q * r.Co, bias, r.Co * sizeof(float), hipMemcpyDeviceToDevice, s));
  return 0;
}
int pack_norm(const VaeRow& r, const RowW& o, const float* w, const float* bias, hipStream_t s) {
  if (w) HIP_TRY(hipMemcpyAsync(o.n.g, w, r.Co * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (bias) HIP_TRY(hipMemcpyAsync(o.n.b, bias, r.Co * sizeof(float), hipMemcpyDeviceToDevice, s));
  return 0;
}
int pack_row(const ldmseg_vae* v, const VaeRow& r, const RowW& o, const float* w, const float* bias, hipStream_t s) {
  return r.kind == ROW_CONV3 ? pack_conv3(v, r, o, w, bias, s) : r.kind == ROW_CONVT2 ? pack_convt2(v, r, o, w, bias, s) : pack_norm(r, o, w, bias, s);
}

// the shapes of a row's packings and their buffers in the handle's arena, unfilled
int alloc_row(ldmseg_vae* v, const VaeRow& r, RowW* o) {
  auto floats = [&](float** p, size_t n) {
    void* q;
    TRY(v->arena.alloc(&q, n * sizeof(float)));
    *p = (float*)q;
    return 0;
  };
  if (r.kind == ROW_LN || r.kind == ROW_GN) {
    o->n.C = r.Co;
    TRY(floats(&o->n.g, r.Co));
    return floats(&o->n.b, r.Co);
  }
  ConvW& f = o->w;
  if (r.kind == ROW_CONV3) {
    conv_shape(r.Co, 3, r.cin_pad, r.n_store, EPI_STORE, &f);
  } else {      // [4 phases x Co][Ci], the bias once per phase
    f.N = f.n_valid = 4 * r.Co; f.cin_pad = r.cin_pad; f.taps = 1; f.cout = r.Co;
  }
  TRY(v->arena.alloc(&f.w, convw_floats(f) * esize(v->dt)));
  TRY(floats(&f.bias, f.N));
  if (r.dgrad_epi < 0) return 0;
  const DgradShape d = r.kind == ROW_CONVT2 ? dgrad_convt_shape(r.Ci, r.Co) : r.stride == 2 ? dgrad_conv_s2_shape(r.Co, r.Ci) : dgrad_conv_shape(r.Co, r.Ci, r.dgrad_epi);
  o->d.N = d.N; o->d.n_valid = d.n_valid; o->d.cin_pad = d.cin_pad; o->d.taps = d.taps; o->d.cout = d.cout;
  return v->arena.alloc(&o->d.w, convw_floats(o->d) * sizeof(float));
}

int vae_build(ldmseg_vae* v, const WeightMap& wm) {
  Builder b(*v, wm);
  const ldmseg_vae_cfg& c = v->cfg;
  const int dt = v->dt;
  if (c.in_channels > bke(dt) || c.latent_channels > bke(dt)) return fail(LDMSEG_E_ARG, "too many boundary channels");
  if (c.int_channels % 64 || c.upscale_channels % 64 || c.num_upscalers < 1 || c.num_upscalers > 4)
    return fail(LDMSEG_E_ARG, "unsupported seg-VAE configuration");
  v->enc.rows = encoder_rows(c);
  v->dec.rows = decoder_rows(c);
  for (VaeHalf* h : {&v->enc, &v->dec}) {
    h->w.resize(h->rows.size());
    for (size_t i = 0; i < h->rows.size(); ++i) {
      const VaeRow& r = h->rows[i];
      const float *w, *bias;
      TRY(wm.get(r.prefix + ".weight", weight_numel(r), &w));
      TRY(wm.get(r.prefix + ".bias", r.Co, &bias));
      TRY(alloc_row(v, r, &h->w[i]));
      TRY(pack_row(v, r, h->w[i], w, bias, b.s));
      b.nparams += weight_numel(r) + r.Co;
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

// the half's input, fp32 NCHW [B, C, H, H] * mul + add, as the packed NHWC activation of one K tile
int vae_input(Exec& ex, const float* x, int C, int H, float mul, float add, Act* a) {
  *a = ex.new_act(bke(ex.dt), H, H, true);
  return ex.launch("launch_pack_nchw failed", 4, 0, 0, no_label, [&] { return launch_pack_nchw(x, a->p, ex.B, C, H * H, bke(ex.dt), mul, add, ex.dt, ex.s); });
}

// what a backward keeps of its half's forward: in[i] = the input of row i (the head's too), pre[i] = the output of a conv + SiLU row before the SiLU
struct Keep {
  std::vector<Act> in, pre;
  explicit Keep(size_t rows) : in(rows), pre(rows) {}
};
// The forward walk of a half from its packed input `h` up to the head conv's input *out (the GroupNorm's output).  keep null: the
// launches of a forward - SiLU in the conv's epilogue, LayerNorm in place.  With keep, what a backward replays: a conv + SiLU row is
// the SiLU-less conv, whose output stays, and one silu_fwd launch; LayerNorm out of place; every row's input retained.
int vae_trunk(Exec& ex, const VaeHalf& half, Act h, Keep* keep, Act* out) {
  for (size_t i = 0;; ++i) {
    if (keep) keep->in[i] = h;
    if (i + 1 == half.rows.size()) break;
    const VaeRow& r = half.rows[i];
    const RowW& w = half.w[i];
    Act o;
    if (r.kind == ROW_CONV3) {
      TRY(ex.conv(w.w, h, &o, {.stride = r.stride, .silu = keep ? 0 : r.silu}));
      if (keep && r.silu) {
        const Act u = keep->pre[i] = o;
        o = ex.new_act(u.C, u.H, u.W, true);
        const size_t n = (size_t)ex.B * u.H * u.W * u.C;
        TRY(ex.launch("launch_silu_fwd failed", 4, 0, 8.0 * n, no_label, [&] { return launch_silu_fwd((const float*)u.p, (float*)o.p, n, ex.s); }));
      }
    } else if (r.kind == ROW_CONVT2) {
      o = ex.new_act(r.Co, 2 * h.H, 2 * h.W, true);
      TRY(ex.gemm(w.w, h.p, h.C, h.H, h.W, o.p, EPI_CONVT2));
    } else if (r.kind == ROW_LN) {
      TRY(ex.layernorm(w.n, h, r.eps, r.silu, &o, !keep));      // (kept: the transposed conv's own output is the backward's input)
    } else {
      TRY(ex.groupnorm(w.n, h, nullptr, r.eps, r.silu, &o));
    }
    h = o;
  }
  *out = h;
  return 0;
}

// the decoder on an executor that is already set up (the reconstruct chain runs encoder and decoder on ONE workspace pass): trunk, head, tail
int vae_decode_body(Exec& ex, ldmseg_vae* v, const float* z, float z_scale, int L, const DecodeTail& tail) {
  const int B = ex.B;
  hipStream_t s = ex.s;
  const int dt = v->dt;
  const ldmseg_vae_cfg& c = v->cfg;
  Act zin, g;
  TRY(vae_input(ex, z, c.latent_channels, L, z_scale, 0.f, &zin));
  TRY(vae_trunk(ex, v->dec, zin, nullptr, &g));
  const ConvW& head = v->dec.w.back().w;
  const int H4 = g.H, W4 = g.W, Co = c.out_channels;
  if (tail.kind == DecodeTail::LOGITS) return ex.gemm(head, g.p, g.C, H4, W4, tail.logits, EPI_NCHW_F32);
  // every other tail reads NHWC logits at 4L
  Act lo = ex.new_act(Co, H4, W4, false);
  TRY(ex.gemm(head, g.p, g.C, H4, W4, lo.p, EPI_STORE));
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

// ---- the decoder's backward.  One planned pass: the decoder's trunk again, keeping what the backward reads (the
// logits themselves are not needed), then the chain from d loss / d logits down to every parameter gradient asked for (g[2 i],
// g[2 i + 1]: weight and bias of row i; null = skipped) and to grad_z.
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
  const std::vector<VaeRow>& rows = v->dec.rows;
  const std::vector<RowW>& w = v->dec.w;
  const int head = (int)rows.size() - 1, gn = head - 1;      // rows: conv_in, (transposed conv, LayerNorm) per upscaler, GroupNorm, head
  const int Cu = c.upscale_channels, Co = c.out_channels;
  Keep keep(rows.size());
  Act zin, gact;
  TRY(vae_input(ex, z, c.latent_channels, L, z_scale, 0.f, &zin));
  TRY(vae_trunk(ex, v->dec, zin, &keep, &gact));
  // ---- backward
  Workspace* ws = ex.ws;
  const Act& h = keep.in[gn];
  const int H4 = h.H, W4 = h.W, P4 = B * H4 * W4;
  const int Cop = (int)rup(Co, bke(dt));
  float* dyp = (float*)ws->scratch((size_t)P4 * Cop * sizeof(float));
  TRY(ex.launch("launch_pack_nchw failed", 4, 0, 0, [] { return std::string("pack grad_logits"); }, [&] { return launch_pack_nchw(grad_logits, dyp, B, Co, H4 * W4, Cop, 1.f, 0.f, dt, s); }));
  TRY(run_wgrad(ex, {dyp, Cop, Cop, (const float*)gact.p, Cu, H4, W4, 9, 0, Co, Cu, 0}, g[2 * head]));
  TRY(run_colsum(ex, dyp, Cop, P4, 1, 0, Co, g[2 * head + 1]));
  Act dg = ex.new_act(Cu, H4, W4, false);
  TRY(ex.gemm(w[head].d, dyp, Cop, H4, W4, dg.p, EPI_STORE));
  Act dh = ex.new_act(Cu, H4, W4, false);
  {
    float* scratch = (float*)ws->scratch(gn_bwd_scratch_bytes(B, Cu));
    TRY(ex.launch("launch_gn_silu_bwd failed", 2, 0, 4.0 * P4 * Cu * 4.0, [&] { return "gn_silu_bwd HW=" + std::to_string(H4 * W4) + " C=" + std::to_string(Cu); }, [&] {
      return launch_gn_silu_bwd((const float*)h.p, (const float*)dg.p, w[gn].n.g, w[gn].n.b, (float*)dh.p, g[2 * gn], g[2 * gn + 1], B, H4 * W4, Cu,
                                rows[gn].eps, scratch, s);
    }));
  }
  for (int ln = gn - 1; ln > 0; ln -= 2) {           // the upscalers, last first: rows ln - 1 (transposed conv) and ln (LayerNorm2d + SiLU)
    const int ct = ln - 1;
    const Act& x = keep.in[ct];                      // the transposed conv's input, on the low-resolution map
    const Act& pre = keep.in[ln];                    // ... and its output
    const int Pl = B * x.H * x.W, M = 4 * Pl;
    // LayerNorm2d + SiLU backward; its result is stored phase-major [B, H, W, 2x2, Cu]: both transposed-conv gradients read it as
    // a [Pl][4 Cu] matrix without a repack
    Act dpre = ex.new_act(Cu, pre.H, pre.W, false);
    {
      float* scratch = (float*)ws->scratch(ln_bwd_scratch_bytes(M, Cu));
      TRY(ex.launch("launch_ln_silu_bwd failed", 3, 0, 3.0 * M * Cu * 4.0, [&] { return "ln_silu_bwd M=" + std::to_string(M) + " C=" + std::to_string(Cu); }, [&] {
        return launch_ln_silu_bwd((const float*)pre.p, (const float*)dh.p, w[ln].n.g, w[ln].n.b, (float*)dpre.p, g[2 * ln], g[2 * ln + 1], M, Cu,
                                  rows[ln].eps, 1, pre.H, pre.W, scratch, s);
      }));
    }
    TRY(run_wgrad(ex, {(const float*)dpre.p, 4 * Cu, 4 * Cu, (const float*)x.p, x.C, x.H, x.W, 1, 1, 4 * Cu, x.C, Cu}, g[2 * ct]));
    TRY(run_colsum(ex, (const float*)dpre.p, 4 * Cu, Pl, 4, Cu, Cu, g[2 * ct + 1]));
    Act dx = ex.new_act(x.C, x.H, x.W, false);
    TRY(ex.gemm(w[ct].d, dpre.p, 4 * Cu, x.H, x.W, dx.p, EPI_STORE));
    dh = dx;
  }
  const int P0 = B * L * L, Ci = c.int_channels;
  TRY(run_wgrad(ex, {(const float*)dh.p, Ci, Ci, (const float*)zin.p, zin.C, L, L, 9, 0, Ci, c.latent_channels, 0}, g[0]));
  TRY(run_colsum(ex, (const float*)dh.p, Ci, P0, 1, 0, Ci, g[1]));
  if (grad_z) {
    TRY(ex.gemm(w[0].d, dh.p, Ci, L, L, grad_z, rows[0].dgrad_epi));
    if (z_scale != 1.0f)     // decode(z, z_scale) feeds z * z_scale
      TRY(ex.launch("launch_axpby failed", 4, 0, 0, no_label, [&] { return launch_axpby(grad_z, z_scale, 0.f, grad_z, (size_t)P0 * c.latent_channels, s); }));
  }
  return 0;
}

// ---- the encoder's backward.  One planned pass: the encoder's trunk again, keeping every row's input and the
// pre-activation u of the four conv + SiLU rows (the moments themselves are not needed), then the chain from d loss / d moments down
// to every parameter gradient asked for (g[2 i], g[2 i + 1]: weight and bias of row i; null = skipped).  The chain stops below the
// lowest row a gradient is asked of; the input is data.
int vae_encode_backward_body(Exec& ex, ldmseg_vae* v, const float* x, float mul, float add, int H, const float* grad_moments, float* const* g) {
  const int B = ex.B;
  hipStream_t s = ex.s;
  const int dt = v->dt;
  const ldmseg_vae_cfg& c = v->cfg;
  const std::vector<VaeRow>& rows = v->enc.rows;
  const std::vector<RowW>& w = v->enc.w;
  const int R = (int)rows.size(), head = R - 1, gn = R - 2;      // rows: the convs 0 .. gn - 1, GroupNorm, head
  int lowest = R;                                  // the lowest row whose parameters are asked for
  for (int i = head; i >= 0; --i)
    if (g[2 * i] || g[2 * i + 1]) lowest = i;
  if (lowest == R) return 0;
  Keep keep(rows.size());
  Act xin, hin;
  TRY(vae_input(ex, x, c.in_channels, H, mul, add, &xin));
  TRY(vae_trunk(ex, v->enc, xin, &keep, &hin));
  // ---- backward: the running gradient alternates between two buffers of the largest activation's size
  Workspace* ws = ex.ws;
  const Act& h7 = keep.in[gn];
  const int l8 = h7.H, P8 = B * l8 * l8, Cm = (int)rup(rows[head].Co, bke(dt)), Ci8 = c.int_channels;
  size_t gmax = (size_t)P8 * Ci8;
  for (int k = 1; k < gn; ++k) gmax = std::max(gmax, (size_t)B * keep.in[k].H * keep.in[k].W * keep.in[k].C);
  float* gb[2] = {(float*)ws->scratch(gmax * sizeof(float)), (float*)ws->scratch(gmax * sizeof(float))};
  float* dm = (float*)ws->scratch((size_t)P8 * Cm * sizeof(float));
  TRY(ex.launch("launch_pack_nchw failed", 4, 0, 0, [] { return std::string("pack grad_moments"); }, [&] { return launch_pack_nchw(grad_moments, dm, B, rows[head].Co, l8 * l8, Cm, 1.f, 0.f, dt, s); }));
  TRY(run_wgrad(ex, {dm, Cm, Cm, (const float*)hin.p, Ci8, l8, l8, 9, 0, rows[head].Co, Ci8, 0, 1, kWgradByWidth}, g[2 * head]));
  TRY(run_colsum(ex, dm, Cm, P8, 1, 0, rows[head].Co, g[2 * head + 1]));
  if (lowest == head) return 0;
  TRY(ex.gemm(w[head].d, dm, Cm, l8, l8, gb[0], rows[head].dgrad_epi));
  {
    const size_t m = ws->mark();
    float* scratch = (float*)ws->scratch(gn_bwd_scratch_bytes(B, Ci8));
    TRY(ex.launch("launch_gn_silu_bwd failed", 2, 0, 4.0 * P8 * Ci8 * 4.0, [&] { return "gn_silu_bwd HW=" + std::to_string(l8 * l8) + " C=" + std::to_string(Ci8); }, [&] {
      return launch_gn_silu_bwd((const float*)h7.p, gb[0], w[gn].n.g, w[gn].n.b, gb[1], g[2 * gn], g[2 * gn + 1], B, l8 * l8, Ci8, rows[gn].eps,
                                scratch, s);
    }));
    ws->reset(m);
  }
  int cur = 1;                                   // gb[cur] = d loss / d (output of row k before its SiLU)
  for (int k = gn - 1; k >= lowest; --k) {
    const Act& xi = keep.in[k];                  // the row's input, on the map H x W of X
    const int Co = rows[k].Co, st = rows[k].stride;
    const int Ho = conv_out_dim(xi.H, st), Wo = conv_out_dim(xi.W, st), Po = B * Ho * Wo;
    TRY(run_wgrad(ex, {gb[cur], Co, Co, (const float*)xi.p, xi.C, xi.H, xi.W, 9, 0, Co, rows[k].Ci, 0, st, kWgradByWidth}, g[2 * k]));
    TRY(run_colsum(ex, gb[cur], Co, Po, 1, 0, Co, g[2 * k + 1]));
    if (k == lowest) break;
    TRY(ex.gemm(w[k].d, gb[cur], Co, Ho, Wo, gb[1 - cur], rows[k].dgrad_epi));      // (stride 2: the four phases, scattered)
    cur = 1 - cur;
    if (rows[k - 1].silu) {                      // the input was SiLU(u[k - 1]): in place
      const size_t n = (size_t)B * xi.H * xi.W * xi.C;
      TRY(ex.launch("launch_silu_bwd failed", 4, 0, 12.0 * n, no_label, [&] { return launch_silu_bwd((const float*)keep.pre[k - 1].p, gb[cur], gb[cur], n, s); }));
    }
  }
  return 0;
}

// the encoder on an executor that is already set up: trunk, then the head straight into the caller's moments
int vae_encode_body(Exec& ex, ldmseg_vae* v, const float* x, float mul, float add, int H, float* moments) {
  Act xin, g;
  TRY(vae_input(ex, x, v->cfg.in_channels, H, mul, add, &xin));
  TRY(vae_trunk(ex, v->enc, xin, nullptr, &g));
  return ex.gemm(v->enc.w.back().w, g.p, g.C, g.H, g.W, moments, EPI_NCHW_F32);
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
  return ex.gemm(v->quant, c8.p, c8.C, h.H, h.W, moments, EPI_NCHW_F32);
}

// ---- what the ABI's pairs share.  ldmseg_vae_{decode,encode}_backward: the argument checks, the gradients by slot, one planned pass
// around `chain` (the half's backward body on an executor).  tensors_ok: the entry's input and output-gradient pointers are there.
template <typename Chain>
int vae_backward(ldmseg_vae* h, bool decoder, bool tensors_ok, bool shape_ok, const char* shape_msg, int B, int n, const char* const* names,
                 float* const* grad_ptrs, const int64_t* numels, void* stream, Chain&& chain) {
  g_err.clear();
  if (!h || !tensors_ok) return fail(LDMSEG_E_ARG, "null argument");
  if (n < 0 || (n > 0 && (!names || !grad_ptrs || !numels))) return fail(LDMSEG_E_ARG, "null argument");
  if (h->dt != DT_F32)
    return fail(LDMSEG_E_ARG, std::string("the ") + (decoder ? "decoder" : "encoder") + " backward needs an fp32-storage handle (compute_dtype fp32 or bf16x3), not bf16");
  if (!decoder && !encoder_backward_ok(h->cfg)) return fail(LDMSEG_E_ARG, "the encoder backward needs block_out_channels and int_channels that are multiples of 32");
  if (!shape_ok) return fail(LDMSEG_E_SHAPE, shape_msg);
  std::vector<void*> g;
  TRY(by_slot(decoder ? h->dec.rows : h->enc.rows, decoder, n, names, (void* const*)grad_ptrs, numels, true, &g));
  DeviceGuard dg(h->cfg.device);
  return plan_and_run(*h, nullptr, [&](bool dry, size_t scratch_base) {
    Exec ex = make_exec(*h, B, (hipStream_t)stream, dry, scratch_base);
    return chain(ex, (float* const*)g.data());
  });
}
// ldmseg_vae_load_{decoder,encoder}: the given tensors of that half through the build's pack path; absent keys are left alone
int vae_load(ldmseg_vae* h, bool decoder, int n, const char* const* names, const void* const* dev_ptrs, const int64_t* numels, void* stream) {
  g_err.clear();
  if (!h || n < 0 || (n > 0 && (!names || !dev_ptrs || !numels))) return fail(LDMSEG_E_ARG, "null argument");
  const VaeHalf& half = decoder ? h->dec : h->enc;
  std::vector<void*> t;
  TRY(by_slot(half.rows, decoder, n, names, (void* const*)dev_ptrs, numels, false, &t));
  DeviceGuard dg(h->cfg.device);
  for (size_t i = 0; i < half.rows.size(); ++i)
    TRY(pack_row(h, half.rows[i], half.w[i], (const float*)t[2 * i], (const float*)t[2 * i + 1], (hipStream_t)stream));
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
  return vae_backward(h, true, z && grad_logits, B >= 1 && L >= 1, "bad B/L", B, n, names, grad_ptrs, numels, stream,
                      [&](Exec& ex, float* const* g) { return vae_decode_backward_body(ex, h, z, z_scale, L, grad_logits, grad_z, g); });
}

int ldmseg_vae_load_decoder(ldmseg_vae* h, int n, const char* const* names, const void* const* dev_ptrs, const int64_t* numels, void* stream) {
  return vae_load(h, true, n, names, dev_ptrs, numels, stream);
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
  return vae_backward(h, false, x && grad_moments, B >= 1 && H >= 8 && H % 8 == 0, "H must be a multiple of 8", B, n, names, grad_ptrs, numels, stream,
                      [&](Exec& ex, float* const* g) { return vae_encode_backward_body(ex, h, x, in_mul, in_add, H, grad_moments, g); });
}

int ldmseg_vae_load_encoder(ldmseg_vae* h, int n, const char* const* names, const void* const* dev_ptrs, const int64_t* numels, void* stream) {
  return vae_load(h, false, n, names, dev_ptrs, numels, stream);
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
