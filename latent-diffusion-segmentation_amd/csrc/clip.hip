// The two CLIP towers of libldmseg_hip.so with their C ABI (include/ldmseg_hip.h).  The runtime underneath: runtime.h.
#include "runtime.h"

using namespace ldmseg;
using namespace ldmseg::rt;

// =================================================================== CLIP vision encoder
// transformers CLIPVisionModel(/WithProjection) - the image descriptor of the clip_image / clip_image_proj modes
// (ldmseg/models/descriptors.py:15-76).  Row-local kernels: clip_vision.hip; every GEMM and the attention: the UNet's kernels.
struct ClipLayerW { ConvW qkv, out, fc1, fc2; };
struct ldmseg_clip_vision : HandleBase {
  ldmseg_clip_vision_cfg cfg{};
  int T = 0, Kpad = 0;          // tokens per image; K of the patch GEMM (3 * patch^2 rounded up to whole 128-byte lines)
  ConvW patch;
  float* cls = nullptr;
  float* pos = nullptr;
  NormW pre, post;
  std::vector<ClipLayerW> layers;
  float* wproj = nullptr;       // visual_projection [projection_dim][hidden] fp32 (GEMV on the B pooled rows)
};

// transformers CLIPTextModel - SD-1.x's text_encoder, the conditioning model of image_descriptors `none`
// (ldmseg/models/descriptors.py:98-103, called at trainers_ldm_cond.py:1108-1119).  Row-local kernels: clip_text.hip; the blocks are
// the vision tower's, with the causal form of the attention.
struct ldmseg_clip_text : HandleBase {
  ldmseg_clip_text_cfg cfg{};
  float* tok = nullptr;         // token_embedding [vocab][hidden] fp32
  float* pos = nullptr;         // position_embedding [max_positions][hidden] fp32
  NormW fin;                    // final_layer_norm
  std::vector<ClipLayerW> layers;
};

namespace {

constexpr float kQuickGelu = 1.702f;   // quick_gelu(x) = x * sigmoid(1.702 x) = silu(1.702 x) / 1.702

// Linear [N][K] with every weight scaled by `scale` (the bias is not)
int build_scaled_linear(Builder& b, const std::string& prefix, int N, int K, float scale, ConvW* out) {
  const int dt = b.dt;
  const float* w;
  TRY(b.wm->get(prefix + ".weight", (int64_t)N * K, &w));
  const int Npad = (int)rup(N, igemm_pick_bn(N, EPI_STORE));
  out->N = Npad; out->n_valid = N; out->cin_pad = K; out->taps = 1; out->cout = N;
  float* cs;
  HIP_TRY(hipMalloc((void**)&cs, (size_t)K * sizeof(float))); b.temps.push_back(cs);
  {
    const std::vector<float> hv(K, scale);
    HIP_TRY(hipMemcpy(cs, hv.data(), (size_t)K * sizeof(float), hipMemcpyHostToDevice));
  }
  std::vector<int> map(Npad, -1);
  for (int r = 0; r < N; ++r) map[r] = r;
  int* dmap;
  TRY(b.upload_ints(map, &dmap));
  TRY(b.arena->alloc(&out->w, (size_t)Npad * K * esize(dt)));
  TRY(launch_repack_rows_scaled(w, out->w, dmap, Npad, K, cs, dt, b.s));
  b.weights(out->w, (size_t)Npad * K);
  b.nparams += (int64_t)N * K;
  const std::string bkey = prefix + ".bias";
  return b.padded_bias(&bkey, N, Npad, &out->bias);
}

// encoder.layers.{i} of a CLIP tower (vision and text hold the same pre-norm block under the same keys)
int clip_build_layers(Builder& b, const WeightMap& wm, int C, int I, int num_layers, std::vector<ClipLayerW>* layers) {
  layers->resize(num_layers);
  // out = scale * Linear(LayerNorm(x)) as one folded-LayerNorm launch, N padded with zero rows to the 160-column tile the folded
  // instantiations have.  The LayerNorm's gamma / beta are read where the caller's tensors lie: they are needed at build time only.
  auto ln_linear = [&](const std::string& ln, const std::vector<std::string>& lin, int Nper, float scale, ConvW* out) -> int {
    const float *gamma, *beta;
    TRY(wm.get(ln + ".weight", C, &gamma));
    TRY(wm.get(ln + ".bias", C, &beta));
    b.nparams += 2 * (int64_t)C;
    std::vector<std::string> wk, bk;
    for (const std::string& l : lin) { wk.push_back(l + ".weight"); bk.push_back(l + ".bias"); }
    const int Nreal = (int)lin.size() * Nper;
    return b.ln_linear(gamma, beta, wk, bk, Nper, C, (int)rup(Nreal, 160), Nreal, nullptr, scale, out);
  };
  for (int i = 0; i < num_layers; ++i) {
    const std::string p = "encoder.layers." + std::to_string(i) + ".";
    ClipLayerW& l = (*layers)[i];
    TRY(ln_linear(p + "layer_norm1", {p + "self_attn.q_proj", p + "self_attn.k_proj", p + "self_attn.v_proj"}, C, 1.f, &l.qkv));
    TRY(b.conv(p + "self_attn.out_proj", C, C, 1, C, &l.out));
    // quick_gelu on the SiLU epilogue: fc1 scaled by 1.702, fc2's weights by 1 / 1.702
    TRY(ln_linear(p + "layer_norm2", {p + "mlp.fc1"}, I, kQuickGelu, &l.fc1));
    TRY(build_scaled_linear(b, p + "mlp.fc2", C, I, 1.f / kQuickGelu, &l.fc2));
  }
  return 0;
}

// The blocks on the residual stream h [ex.B * T][C] (T = h.H), in place.  attn: the self-attention launcher on the fused q | k | v
// rows - launch_attention for the vision tower, launch_attention_causal for the text tower; everything else is the same launches.
using ClipAttn = int (*)(const void* qkv, void* out, int B, int N, int C, int heads, int dtype, hipStream_t s);
int clip_run_layers(Exec& ex, const std::vector<ClipLayerW>& layers, const Act& h, int I, int heads, ClipAttn attn) {
  Workspace* ws = ex.ws;
  hipStream_t s = ex.s;
  const int dt = ex.dt, B = ex.B, C = h.C, T = h.H, M = B * T;
  const size_t es = esize(dt);
  for (const ClipLayerW& l : layers) {
    const size_t m = ws->mark();
    float* stats = (float*)ws->scratch((size_t)M * 2 * sizeof(float));
    void* qkv = ws->scratch((size_t)M * 3 * C * es);
    void* att = ws->scratch((size_t)M * C * es);
    TRY(ex.rowstats(h, 1e-5f, stats));
    TRY(ex.linear(l.qkv, h.p, C, T, 1, qkv, 3 * C, {stats}));                       // layer_norm1 -> q | k | v
    TRY(ex.launch("self-attention launch (head dim 64) failed", 1, 4.0 * B * (double)T * T * C, 4.0 * M * C * es,
                  [&] { return "clip N=" + std::to_string(T) + " C=" + std::to_string(C); },
                  [&] { return attn(qkv, att, B, T, C, heads, ex.x3 ? 2 : dt, s); }));
    TRY(ex.linear(l.out, att, C, T, 1, h.p, C, {nullptr, h.p}));                    // h += out_proj(att)
    ws->reset(m);
    stats = (float*)ws->scratch((size_t)M * 2 * sizeof(float));
    void* ff = ws->scratch((size_t)M * I * es);
    TRY(ex.rowstats(h, 1e-5f, stats));
    TRY(ex.linear(l.fc1, h.p, C, T, 1, ff, I, {stats, nullptr, EPI_STORE, 1}));     // silu(1.702 fc1(layer_norm2(h)))
    TRY(ex.linear(l.fc2, ff, I, T, 1, h.p, C, {nullptr, h.p}));                      // h += fc2(.) / 1.702
    ws->reset(m);
  }
  return 0;
}

int clip_build(ldmseg_clip_vision* v, const WeightMap& wm) {
  Builder b(*v, wm);
  const ldmseg_clip_vision_cfg& c = v->cfg;
  const int C = c.hidden_size, I = c.intermediate_size, P = c.patch_size;
  v->T = (c.image_size / P) * (c.image_size / P) + 1;
  v->Kpad = (int)rup((size_t)3 * P * P, 64);
  // patch_embedding [C][3][P][P] is a Linear over k = (channel, dy, dx): [C][3 P P] padded to [C][Kpad]
  TRY(b.conv("embeddings.patch_embedding", C, 3 * P * P, 1, v->Kpad, &v->patch, false));
  TRY(b.f32_copy("embeddings.class_embedding", C, &v->cls));
  TRY(b.f32_copy("embeddings.position_embedding.weight", (int64_t)v->T * C, &v->pos));
  TRY(b.norm("pre_layrnorm", C, &v->pre));
  TRY(clip_build_layers(b, wm, C, I, c.num_layers, &v->layers));
  TRY(b.norm("post_layernorm", C, &v->post));
  if (c.projection_dim > 0) TRY(b.f32_copy("visual_projection.weight", (int64_t)c.projection_dim * C, &v->wproj));
  return b.finish(*v);
}

int clip_forward_impl(ldmseg_clip_vision* v, const float* img, int B, int H, int W, const float* mean, const float* std,
                      int resample, float* last_hidden, float* image_embeds, hipStream_t s, bool dry, size_t scratch_base) {
  Workspace* ws = &v->ws;
  Exec ex = make_exec(*v, B, s, dry, scratch_base);
  const ldmseg_clip_vision_cfg& c = v->cfg;
  const int dt = v->dt, C = c.hidden_size, I = c.intermediate_size, T = v->T, NP = T - 1, M = B * T;
  const size_t es = esize(dt);
  Act h;
  h.C = C; h.H = T; h.W = 1;
  h.p = ws->persist((size_t)M * C * es);
  {
    const size_t m = ws->mark();
    void* rows = ws->scratch((size_t)B * NP * v->Kpad * es);
    void* pe = ws->scratch((size_t)B * NP * C * es);
    TRY(ex.launch("launch_clip_patch_rows failed", 4, 0, 0, no_label, [&] { return launch_clip_patch_rows(img, rows, B, H, W, c.image_size, c.patch_size, v->Kpad, mean, std, resample, dt, s); }));
    TRY(ex.linear(v->patch, rows, v->Kpad, NP, 1, pe, C));
    TRY(ex.launch("launch_clip_tokens failed", 3, 0, 2.0 * M * C * es, no_label, [&] { return launch_clip_tokens(pe, v->cls, v->pos, v->pre.g, v->pre.b, h.p, B, T, C, 1e-5f, dt, s); }));
    ws->reset(m);
  }
  TRY(clip_run_layers(ex, v->layers, h, I, c.num_heads, launch_attention));
  if (last_hidden)
    TRY(ex.launch("launch_clip_rows_to_f32 failed", 4, 0, 0, no_label, [&] { return launch_clip_rows_to_f32(h.p, last_hidden, (size_t)M * C, dt, s); }));
  if (image_embeds) {
    float* pooled = (float*)ws->scratch((size_t)B * C * sizeof(float));
    TRY(ex.launch("image_embeds (pooled LayerNorm, projection) failed", 4, 0, 0, no_label, [&] {
      const int r = launch_clip_pooled_ln(h.p, v->post.g, v->post.b, pooled, B, T, C, 1e-5f, dt, s);
      return r ? r : launch_small_linear(pooled, v->wproj, nullptr, image_embeds, B, C, c.projection_dim, 0, 0, s);
    }));
  }
  return 0;
}

int clip_forward_checked(ldmseg_clip_vision* v, const float* img, int B, int H, int W, const float* mean, const float* std,
                         int resample, float* last_hidden, float* image_embeds, hipStream_t s) {
  if (!v || !img) return fail(LDMSEG_E_ARG, "null argument");
  if (B < 1 || H < 1 || W < 1 || (long)B * v->T > (1 << 22)) return fail(LDMSEG_E_SHAPE, "B, H, W must be >= 1 (and B * tokens <= 2^22)");
  if (image_embeds && !v->wproj) return fail(LDMSEG_E_ARG, "image_embeds requested from a handle without visual_projection");
  // the plan covers both outputs, so that it does not depend on which the caller asked for
  float* const any = (float*)(uintptr_t)0x1000;
  const PlanKey key{B};
  return plan_and_run(*v, &key, [&](bool dry, size_t scratch_base) {
    return clip_forward_impl(v, img, B, H, W, mean, std, resample, dry ? any : last_hidden, dry ? (v->wproj ? any : nullptr) : image_embeds, s,
                             dry, scratch_base);
  });
}

int clip_text_build(ldmseg_clip_text* v, const WeightMap& wm) {
  Builder b(*v, wm);
  const ldmseg_clip_text_cfg& c = v->cfg;
  const int C = c.hidden_size;
  TRY(b.f32_copy("embeddings.token_embedding.weight", (int64_t)c.vocab_size * C, &v->tok));
  TRY(b.f32_copy("embeddings.position_embedding.weight", (int64_t)c.max_positions * C, &v->pos));
  TRY(clip_build_layers(b, wm, C, c.intermediate_size, c.num_layers, &v->layers));
  TRY(b.norm("final_layer_norm", C, &v->fin));
  return b.finish(*v);
}

int clip_text_forward_impl(ldmseg_clip_text* v, const int64_t* ids, int R, int T, float* last_hidden, hipStream_t s, bool dry,
                           size_t scratch_base) {
  Workspace* ws = &v->ws;
  Exec ex = make_exec(*v, R, s, dry, scratch_base);
  const ldmseg_clip_text_cfg& c = v->cfg;
  const int dt = v->dt, C = c.hidden_size, M = R * T;
  const size_t es = esize(dt);
  Act h;
  h.C = C; h.H = T; h.W = 1;
  h.p = ws->persist((size_t)M * C * es);
  TRY(ex.launch("launch_clip_text_tokens failed", 3, 0, (double)M * C * (8 + es), no_label, [&] { return launch_clip_text_tokens(ids, v->tok, v->pos, h.p, R, T, C, c.vocab_size, dt, s); }));
  TRY(clip_run_layers(ex, v->layers, h, c.intermediate_size, c.num_heads, launch_attention_causal));
  return ex.launch("launch_clip_text_final_ln failed", 3, 0, (double)M * C * (4 + es), no_label, [&] { return launch_clip_text_final_ln(h.p, v->fin.g, v->fin.b, last_hidden, M, C, 1e-5f, dt, s); });
}

}  // namespace

// =================================================================== C ABI
extern "C" {

int ldmseg_clip_vision_create(const ldmseg_clip_vision_cfg* cfg, int n_weights, const char* const* names,
                              const void* const* dev_ptrs, const int64_t* numels, ldmseg_clip_vision** out) {
  auto check = [](const ldmseg_clip_vision_cfg& c) {
    if (c.num_layers < 1 || c.projection_dim < 0) return fail(LDMSEG_E_ARG, "num_layers must be >= 1, projection_dim >= 0");
    if (c.num_heads < 1 || c.hidden_size != 64 * c.num_heads) return fail(LDMSEG_E_SHAPE, "hidden_size / num_heads must be 64 (the head dim the attention kernel is built for here)");
    // (hidden_size is a multiple of 64 by the line above.  1280: the widest row launch_rowstats serves in fp32, and the widest K the
    // folded-LayerNorm GEMMs run at in the UNet - one bound for all modes)
    if (c.hidden_size > 1280) return fail(LDMSEG_E_SHAPE, "hidden_size must be at most 1280");
    if (c.intermediate_size < 64 || c.intermediate_size % 64 != 0) return fail(LDMSEG_E_SHAPE, "intermediate_size must be a multiple of 64");
    if (c.patch_size < 1 || c.image_size < c.patch_size || c.image_size % c.patch_size != 0) return fail(LDMSEG_E_SHAPE, "image_size must be a multiple of patch_size");
    return 0;
  };
  return create_handle(cfg, n_weights, names, dev_ptrs, numels, check, clip_build, false, out);    // (no GroupNorm in a ViT)
}
LDMSEG_HANDLE_ABI(ldmseg_clip_vision)

int ldmseg_clip_vision_forward(ldmseg_clip_vision* h, const float* pixel_values, int B, float* last_hidden, float* image_embeds,
                               void* stream) {
  g_err.clear();
  if (!h) return fail(LDMSEG_E_ARG, "null handle");
  DeviceGuard dg(h->cfg.device);
  return clip_forward_checked(h, pixel_values, B, h->cfg.image_size, h->cfg.image_size, nullptr, nullptr, 0, last_hidden, image_embeds,
                              (hipStream_t)stream);
}

int ldmseg_clip_vision_describe(ldmseg_clip_vision* h, const float* rgb, int B, int H, int W, const float mean[3],
                                const float std[3], float* last_hidden, float* image_embeds, void* stream) {
  g_err.clear();
  if (!h || !mean || !std) return fail(LDMSEG_E_ARG, "null argument");
  for (int c = 0; c < 3; ++c)
    if (!(std[c] > 0.f)) return fail(LDMSEG_E_ARG, "std must be positive");
  DeviceGuard dg(h->cfg.device);
  return clip_forward_checked(h, rgb, B, H, W, mean, std, 1, last_hidden, image_embeds, (hipStream_t)stream);
}

int ldmseg_clip_text_create(const ldmseg_clip_text_cfg* cfg, int n_weights, const char* const* names,
                            const void* const* dev_ptrs, const int64_t* numels, ldmseg_clip_text** out) {
  auto check = [](const ldmseg_clip_text_cfg& c) {
    if (c.num_layers < 1 || c.vocab_size < 1 || c.max_positions < 1) return fail(LDMSEG_E_ARG, "num_layers, vocab_size and max_positions must be >= 1");
    // (the limits of the vision handle: the same attention, statistics and GEMM kernels run here)
    if (c.num_heads < 1 || c.hidden_size != 64 * c.num_heads) return fail(LDMSEG_E_SHAPE, "hidden_size / num_heads must be 64 (the head dim the attention kernel is built for here)");
    if (c.hidden_size > 1280) return fail(LDMSEG_E_SHAPE, "hidden_size must be at most 1280");
    if (c.intermediate_size < 64 || c.intermediate_size % 64 != 0) return fail(LDMSEG_E_SHAPE, "intermediate_size must be a multiple of 64");
    return 0;
  };
  return create_handle(cfg, n_weights, names, dev_ptrs, numels, check, clip_text_build, false, out);
}
LDMSEG_HANDLE_ABI(ldmseg_clip_text)

int ldmseg_clip_text_forward(ldmseg_clip_text* h, const int64_t* input_ids_dev, int R, int T, float* last_hidden, void* stream) {
  g_err.clear();
  if (!h || !input_ids_dev || !last_hidden) return fail(LDMSEG_E_ARG, "null argument");
  if (R < 1 || (long)R * h->cfg.max_positions > (1 << 22)) return fail(LDMSEG_E_SHAPE, "R must be >= 1 (and R * max_positions <= 2^22)");
  if (T < 1 || T > h->cfg.max_positions) return fail(LDMSEG_E_SHAPE, "T must be in [1, max_positions]");
  DeviceGuard dg(h->cfg.device);
  const PlanKey key{R, T};
  return plan_and_run(*h, &key, [&](bool dry, size_t scratch_base) {
    return clip_text_forward_impl(h, input_ids_dev, R, T, last_hidden, (hipStream_t)stream, dry, scratch_base);
  });
}

}  // extern "C"
