// The UNet's weight repacking: the state dict -> the packed matrices, streams and tables of ldmseg_unet (create time).
#include "unet.h"

namespace ldmseg::rt {

namespace {

// attn2 of a cross-attention handle: norm2 folded into to_q like norm1 into q|k|v; to_k | to_v as one [2C][768] matrix
int build_attn2(Builder& b, const std::string& tb, int C, TransformerW* t) {
  const int dt = b.dt;
  TRY(b.norm(tb + "norm2", C, &t->ln2));
  TRY(b.ln_linear(t->ln2.g, t->ln2.b, {tb + "attn2.to_q.weight"}, {}, C, C, (int)rup(C, igemm_pick_bn(C, EPI_STORE)), C, nullptr, 0.f, &t->q2));
  {
    ConvW& k = t->kv2;
    const int Np = (int)rup(2 * C, igemm_pick_bn(2 * C, EPI_STORE));
    k.N = Np; k.n_valid = 2 * C; k.cin_pad = kCrossDim; k.taps = 1; k.cout = 2 * C;
    std::vector<int> map(Np);
    for (int r = 0; r < Np; ++r) map[r] = r < C ? r : -1;
    int* dmap;
    TRY(b.upload_ints(map, &dmap));
    TRY(b.arena->alloc(&k.w, (size_t)Np * kCrossDim * esize(dt)));
    b.weights(k.w, (size_t)Np * kCrossDim);
    const float *wk, *wv;
    TRY(b.wm->get(tb + "attn2.to_k.weight", (int64_t)C * kCrossDim, &wk));
    TRY(b.wm->get(tb + "attn2.to_v.weight", (int64_t)C * kCrossDim, &wv));
    // rows [0, C) <- to_k, [C, 2C) <- to_v, the padding rows behind them zero (map -1)
    TRY(launch_repack_rows(wk, k.w, dmap, C, kCrossDim, dt, b.s));
    TRY(launch_repack_rows(wv, (char*)k.w + (size_t)C * kCrossDim * esize(dt), dmap, Np - C, kCrossDim, dt, b.s));
    TRY(b.padded_bias(nullptr, 0, Np, &k.bias));
    b.nparams += (int64_t)2 * C * kCrossDim;
  }
  TRY(b.conv(tb + "attn2.to_out.0", C, C, 1, C, &t->out2));
  return 0;
}

int build_transformer(Builder& b, const std::string& p, int C, TransformerW* t, bool cross = false) {
  t->C = C;
  const int dt = b.dt;
  TRY(b.norm(p + "norm", C, &t->norm));
  TRY(b.conv(p + "proj_in", C, C, 1, C, &t->proj_in));
  const std::string tb = p + "transformer_blocks.0.";
  TRY(b.norm(tb + "norm1", C, &t->ln1));
  // fused q|k|v projection, no bias, with norm1 (LayerNorm) folded in
  TRY(b.ln_linear(t->ln1.g, t->ln1.b, {tb + "attn1.to_q.weight", tb + "attn1.to_k.weight", tb + "attn1.to_v.weight"}, {}, C, C, 3 * C, 3 * C,
                  nullptr, 0.f, &t->qkv));
  TRY(b.conv(tb + "attn1.to_out.0", C, C, 1, C, &t->attn_out));
  if (cross) TRY(build_attn2(b, tb, C, t));
  TRY(b.norm(tb + "norm3", C, &t->ln3));
  // GEGLU projection [8C, C]: rows interleaved in 16-row (a | gate) pairs so one lane owns both halves; norm3 folded in
  {
    const std::vector<int> map = geglu_row_map(4 * C);
    TRY(b.ln_linear(t->ln3.g, t->ln3.b, {tb + "ff.net.0.proj.weight"}, {tb + "ff.net.0.proj.bias"}, 8 * C, C, 8 * C, 4 * C, &map, 0.f, &t->ff1));
  }
  TRY(b.conv(tb + "ff.net.2", C, 4 * C, 1, 4 * C, &t->ff2));
  TRY(b.conv(p + "proj_out", C, C, 1, C, &t->proj_out));
  if (const size_t sb = (dt == DT_BF16 && t->ff1.N == 8 * C && t->ff2.N == C && t->proj_out.N == C) ? mlp_fused_stream_bytes(C) : 0) {
    TRY(b.arena->alloc(&t->mlp_stream, sb));
    TRY(launch_pack_mlp_stream(t->ff1.w, t->ff2.w, t->proj_out.w, t->mlp_stream, C, b.s));
  }
  // proj_out(h + ff.net.2(g)) + x has no nonlinearity between the two Linears (the transformer block ends with the feed-forward's
  // residual, Transformer2DModel.proj_out follows): = [Wp W2 | Wp] [g | h] + (bp + Wp b2) + x.  Same FLOPs (2 M C 5C), one launch
  // and one [M, C] round trip fewer: the levels that do not run the row-local fused kernel hold the chained matrix.
  if (dt == DT_BF16 && !t->mlp_stream && C % 160 == 0 && t->ff2.N == C && t->proj_out.N == C) {
    const float *w2, *b2, *wp, *bp;
    TRY(b.wm->get(tb + "ff.net.2.weight", (int64_t)C * 4 * C, &w2));
    TRY(b.wm->get(tb + "ff.net.2.bias", C, &b2));
    TRY(b.wm->get(p + "proj_out.weight", (int64_t)C * C, &wp));
    TRY(b.wm->get(p + "proj_out.bias", C, &bp));
    void* wcat;
    HIP_TRY(hipMalloc(&wcat, (size_t)C * 5 * C * sizeof(float)));
    b.temps.push_back(wcat);
    void* bcat;
    TRY(b.arena->alloc(&bcat, C * sizeof(float)));
    TRY(launch_chain_weights(wp, w2, b2, bp, (float*)wcat, (float*)bcat, C, b.s));
    std::vector<int> ident(C);
    for (int r = 0; r < C; ++r) ident[r] = r;
    int* dident;
    TRY(b.upload_ints(ident, &dident));
    ConvW& f = t->ffp;
    f.N = C; f.n_valid = C; f.cin_pad = 5 * C; f.taps = 1; f.cout = C;
    TRY(b.arena->alloc(&f.w, (size_t)C * 5 * C * esize(dt)));
    TRY(launch_repack_rows((const float*)wcat, f.w, dident, C, 5 * C, dt, b.s));
    f.bias = (float*)bcat;
  }
  if (const size_t sb = (dt == DT_BF16 && t->proj_in.N == C && t->proj_in.cin_pad == C && t->qkv.N == 3 * C) ? proj_qkv_stream_bytes(C) : 0) {
    TRY(b.arena->alloc(&t->in_stream, sb));
    TRY(launch_pack_proj_qkv_stream(t->proj_in.w, t->qkv.w, t->in_stream, C, b.s));
    void* pb;
    TRY(b.arena->alloc(&pb, (size_t)4 * C * sizeof(float)));
    t->in_bias = (float*)pb;
    HIP_TRY(hipMemcpyAsync(t->in_bias, t->proj_in.bias, (size_t)C * sizeof(float), hipMemcpyDeviceToDevice, b.s));
    HIP_TRY(hipMemcpyAsync(t->in_bias + C, t->qkv.bias, (size_t)3 * C * sizeof(float), hipMemcpyDeviceToDevice, b.s));
  }
  return 0;
}

}  // namespace

int unet_build(ldmseg_unet* u, const WeightMap& wm) {
  Builder b(*u, wm);
  hipStream_t s = b.s;
  const int cp = bke(u->dt);
  if (u->cfg.in_channels > cp) return fail(LDMSEG_E_ARG, "in_channels too large");
  u->sepenc = wm.m.count("conv_in_img.weight") != 0;
  if (u->sepenc && (u->cfg.in_channels != 8 || u->cfg.cross_attention != 0))
    return fail(LDMSEG_E_ARG, "separate image encoder (conv_in_img.*): in_channels must be 8 and cross_attention 0");
  // (separate encoder: conv_in sees the 4 segmentation channels of the 8-channel packed input, i.e. zero weights on the RGB columns -
  // the repack's channel padding - so the main path is the plain 8-channel UNet's launches)
  TRY(b.conv("conv_in", kBlockOut[0], u->sepenc ? 4 : u->cfg.in_channels, 3, cp, &u->conv_in));
  const bool cross = u->cfg.cross_attention != 0;
  if (cross && wm.m.count("encoder_hid_proj.weight"))       // optional (clip_image descriptors, unet.py:121-122)
    TRY(b.conv("encoder_hid_proj", kCrossDim, kHidProjIn, 1, kHidProjIn, &u->hid_proj));
  TRY(b.f32_copy("time_embedding.linear_1.weight", (int64_t)kTimeDim * 320, &u->te1_w));
  TRY(b.f32_copy("time_embedding.linear_1.bias", kTimeDim, &u->te1_b));
  TRY(b.f32_copy("time_embedding.linear_2.weight", (int64_t)kTimeDim * kTimeDim, &u->te2_w));
  TRY(b.f32_copy("time_embedding.linear_2.bias", kTimeDim, &u->te2_b));

  std::vector<std::pair<std::string, const ResnetW*>> made;      // every resnet with its key prefix, in build order: the time_emb_proj tables
  auto resnet = [&](const std::string& p, int cin, int cout, int* off, ResnetW* r) {
    made.emplace_back(p, r);
    return build_resnet(b, p, cin, cout, off, r);
  };
  // down_blocks / down_blocks_additional: two resnets [+ transformers] per level, a stride-2 conv between levels
  auto down = [&](const std::string& name, bool attn2, int* off, ResnetW (&res)[4][2], TransformerW (&attn)[3][2], ConvW (&conv)[3],
                  std::vector<int>* skips) -> int {
    int c = kBlockOut[0];
    for (int i = 0; i < 4; ++i) {
      const std::string p = name + "." + std::to_string(i);
      for (int j = 0; j < 2; ++j) {
        TRY(resnet(p + ".resnets." + std::to_string(j) + ".", c, kBlockOut[i], off, &res[i][j]));
        c = kBlockOut[i];
        if (i < 3) TRY(build_transformer(b, p + ".attentions." + std::to_string(j) + ".", c, &attn[i][j], attn2));
        if (skips) skips->push_back(c);
      }
      if (i < 3) {
        TRY(b.conv(p + ".downsamplers.0.conv", c, c, 3, c, &conv[i]));
        if (skips) skips->push_back(c);
      }
    }
    return 0;
  };
  int temb_off = 0;
  std::vector<int> skip_ch{kBlockOut[0]};
  TRY(down("down_blocks", cross, &temb_off, u->down_res, u->down_attn, u->down_conv, &skip_ch));
  int c = kBlockOut[3];
  TRY(resnet("mid_block.resnets.0.", c, c, &temb_off, &u->mid_res[0]));
  TRY(build_transformer(b, "mid_block.attentions.0.", c, &u->mid_attn, cross));
  TRY(resnet("mid_block.resnets.1.", c, c, &temb_off, &u->mid_res[1]));
  for (int i = 0; i < 4; ++i) {
    const int co = kBlockOut[3 - i];
    for (int j = 0; j < 3; ++j) {
      const std::string p = "up_blocks." + std::to_string(i);
      const int sk = skip_ch.back();
      skip_ch.pop_back();
      TRY(resnet(p + ".resnets." + std::to_string(j) + ".", c + sk, co, &temb_off, &u->up_res[i][j]));
      c = co;
      if (i > 0) TRY(build_transformer(b, p + ".attentions." + std::to_string(j) + ".", c, &u->up_attn[i][j], cross));
    }
    if (i < 3) {
      const std::string key = "up_blocks." + std::to_string(i) + ".upsamplers.0.conv";
      TRY(b.conv(key, c, c, 3, c, &u->up_conv[i]));
      // Upsample2D = nearest x2 then this conv: an output pixel sees only 2 x 2 distinct source pixels, so the conv runs as four
      // 2x2-tap phase convs on the low-resolution map with pre-summed weights (K = 4 C instead of 9 C; igemm.hip UP4)
      ConvW& cw = u->up_conv[i];
      if (u->dt == DT_BF16 && cw.N % 160 == 0 && c % bke(u->dt) == 0) {
        const float* wraw;
        TRY(b.wm->get(key + ".weight", (int64_t)c * c * 9, &wraw));
        TRY(b.arena->alloc(&cw.w_up4, (size_t)16 * cw.N * c * esize(u->dt)));
        TRY(launch_pack_up4(wraw, cw.w_up4, c, c, cw.N, c, u->dt, b.s));
      }
    }
  }
  TRY(b.norm("conv_norm_out", c, &u->norm_out));
  TRY(b.conv("conv_out", 4, c, 3, c, &u->conv_out));

  // the time_emb_proj Linear(1280 -> cout) of resnets made[from, ...) concatenated (all 22 of the UNet: one GEMV per forward)
  auto table = [&](size_t from, int total, float** tw, float** tb) -> int {
    void *pw, *pb;
    TRY(u->arena.alloc(&pw, (size_t)total * kTimeDim * sizeof(float)));
    TRY(u->arena.alloc(&pb, (size_t)total * sizeof(float)));
    *tw = (float*)pw; *tb = (float*)pb;
    for (size_t k = from; k < made.size(); ++k) {
      const ResnetW& r = *made[k].second;
      const float *w, *bias;
      TRY(wm.get(made[k].first + "time_emb_proj.weight", (int64_t)r.cout * kTimeDim, &w));
      TRY(wm.get(made[k].first + "time_emb_proj.bias", r.cout, &bias));
      HIP_TRY(hipMemcpyAsync(*tw + (size_t)r.temb_off * kTimeDim, w, (size_t)r.cout * kTimeDim * sizeof(float), hipMemcpyDeviceToDevice, s));
      HIP_TRY(hipMemcpyAsync(*tb + r.temb_off, bias, r.cout * sizeof(float), hipMemcpyDeviceToDevice, s));
      b.nparams += (int64_t)r.cout * kTimeDim + r.cout;
    }
    return 0;
  };
  u->temb_total = temb_off;
  TRY(table(0, temb_off, &u->tproj_w, &u->tproj_b));
  if (u->sepenc) {
    // conv_in_img reads the RGB half of the same packed 8-channel input: its [320][4][3][3] filters behind four zero input channels
    {
      const float *w4, *bias;
      TRY(wm.get("conv_in_img.weight", (int64_t)kBlockOut[0] * 4 * 9, &w4));
      TRY(wm.get("conv_in_img.bias", kBlockOut[0], &bias));
      void* w8;
      HIP_TRY(hipMalloc(&w8, (size_t)kBlockOut[0] * 8 * 9 * sizeof(float)));
      b.temps.push_back(w8);
      HIP_TRY(hipMemsetAsync(w8, 0, (size_t)kBlockOut[0] * 8 * 9 * sizeof(float), s));
      HIP_TRY(hipMemcpy2DAsync((float*)w8 + 4 * 9, (size_t)8 * 9 * sizeof(float), w4, (size_t)4 * 9 * sizeof(float), (size_t)4 * 9 * sizeof(float),
                               kBlockOut[0], hipMemcpyDeviceToDevice, s));
      WeightMap ext;
      ext.m["conv_in_img.weight"] = {(const float*)w8, (int64_t)kBlockOut[0] * 8 * 9};
      ext.m["conv_in_img.bias"] = {bias, kBlockOut[0]};
      b.wm = &ext;
      const int r = b.conv("conv_in_img", kBlockOut[0], 8, 3, cp, &u->conv_in_img);
      b.wm = &wm;
      TRY(r);
      b.nparams -= (int64_t)kBlockOut[0] * 4 * 9;      // (the four zero channels are not parameters)
    }
    int ioff = 0;
    const size_t first_img = made.size();
    TRY(down("down_blocks_additional", false, &ioff, u->img_res, u->img_attn, u->img_conv, nullptr));
    u->adaptor = wm.m.count("adaptor_layers.0.weight") != 0;
    if (u->adaptor)
      for (int i = 0; i < 4; ++i)
        TRY(b.conv("adaptor_layers." + std::to_string(i), kBlockOut[i], kBlockOut[i], 3, kBlockOut[i], &u->adapt[i], true, 0, EPI_STORE,
                   kBlockOut[i] <= 640));
    // its 8 time_emb_proj (7,040 rows) as a table of their own: they see emb(timestep_img)
    u->temb_img_total = ioff;
    TRY(table(first_img, ioff, &u->tproj_img_w, &u->tproj_img_b));
  }
  return b.finish(*u);
}

}  // namespace ldmseg::rt
