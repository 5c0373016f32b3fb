// The UNet of libldmseg_hip.so: the forward (with the separate image encoder's branch), the two DDIM sampling
// loops and their C ABI (include/ldmseg_hip.h).  The runtime underneath: runtime.h.
#include <cstring>

#include "unet.h"

#pragma clang diagnostic ignored "-Wc++20-designator"      // ConvOpt and its like are filled by field name

using namespace ldmseg;
using namespace ldmseg::rt;

namespace {

int run_resnet(Exec& ex, const ResnetW& r, const Act& x, const Act* skip, const float* temb, int temb_stride, Act* out) {
  Workspace* ws = ex.ws;
  // output first (persist), temporaries on the scratch stack
  const size_t m = ws->mark();
  Act n1, n2, sc;
  TRY(ex.groupnorm(r.norm1, x, skip, 1e-5f, 1, &n1));
  TRY(ex.conv_groupnorm(r.conv1, n1, temb + r.temb_off, temb_stride, r.norm2, 1e-5f, 1, &n2));
  const Act* resid = &x;
  if (r.has_shortcut && ex.conv_xt_ok(r.conv2x, n2, x, skip)) {
    TRY(ex.conv_xt(r.conv2x, n2, x, skip, out));
    ws->reset(m);
    return 0;
  }
  if (r.has_shortcut) {
    TRY(ex.conv(r.shortcut, x, &sc, {.x2 = skip, .persist = false}));
    resid = &sc;
  } else if (skip) {
    return fail(LDMSEG_E_SHAPE, "resnet without shortcut cannot take a concat input");
  }
  TRY(ex.conv(r.conv2, n2, out, {.resid = resid}));
  ws->reset(m);
  return 0;
}

// kv_ctx: this transformer's K|V of the conditioning context [B*S, 2C] (cross-attention handles), null = no attn2
int run_transformer(Exec& ex, const TransformerW& t, const Act& x, Act* out, const void* kv_ctx = nullptr, int S = 0) {
  Workspace* ws = ex.ws;
  const size_t m = ws->mark();
  const int C = t.C, N = x.H * x.W, M = ex.B * N;
  const size_t es = esize(ex.dt);
  Act n, h, qkv, att, ff;
  const bool entry_fused = t.in_stream && proj_qkv_fused_ok(C, M, ex.dt);
  const bool gn_fold = entry_fused && g_gnfold_mode && proj_qkv_gn_fold_ok(N);
  GnFold gf;
  if (gn_fold) TRY(ex.groupnorm_stats(t.norm, x, 1e-6f, &gf));     // the norm's apply pass runs inside the fused entry, on its LDS tile
  else TRY(ex.groupnorm(t.norm, x, nullptr, 1e-6f, 0, &n));
  if (entry_fused) {
    // 320-channel level: proj_in -> norm1 -> q|k|v in one row-local launch (tproj.hip): h is written once and not read back
    h = ex.new_act(C, x.H, x.W, false);
    qkv = ex.new_act(3 * C, x.H, x.W, false);
    TRY(ex.launch("launch_proj_qkv_fused failed", 0, 2.0 * M * 4.0 * C * C, (double)M * C * es * 5.0 + (double)proj_qkv_stream_bytes(C),
                  [&] { return "M=" + std::to_string(M) + " proj_ln_qkv C=" + std::to_string(C); }, [&] {
                    return launch_proj_qkv_fused(gn_fold ? x.p : n.p, h.p, qkv.p, t.in_stream, t.in_bias, igemm_zero_page(), M, C, 1e-5f,
                                                 gn_fold ? &gf : nullptr, ex.s);
                  }));
  } else {
    TRY(ex.conv(t.proj_in, n, &h, {.persist = false}));
    // norm1 is folded into the q|k|v GEMM: one statistics pass over h (mean, rstd per token), the GEMM reads h itself
    float* stats = (float*)ws->scratch((size_t)M * 2 * sizeof(float));
    TRY(ex.rowstats(h, 1e-5f, stats));
    qkv = ex.new_act(3 * C, x.H, x.W, false);
    TRY(ex.linear(t.qkv, h.p, C, x.H, x.W, qkv.p, 3 * C, {stats}));
  }
  att = ex.new_act(C, x.H, x.W, false);
  {
    AttnPlan fp8;
    // long-context level on the fp8 operand path (BASELINE configs[4]); else the dtype's kernel (2 = fp32 tensors, split-bf16 products)
    const bool on_fp8 = attn_self_fp8_level(ex.B, N, C, 8, ex.dt, ex.attn_fp8_min_tokens, attention_knobs(), &fp8);
    void* scratch = on_fp8 ? ws->scratch(fp8.scratch_bytes) : nullptr;
    TRY(ex.launch("launch_attention failed", 1, 4.0 * ex.B * 8 * (double)N * N * (C / 8.0), 4.0 * M * C * es, [&] { return "N=" + std::to_string(N) + " C=" + std::to_string(C); }, [&] {
      return on_fp8 ? launch_attention_fp8(qkv.p, scratch, att.p, ex.B, N, C, 8, ex.s) : launch_attention(qkv.p, att.p, ex.B, N, C, 8, ex.x3 ? 2 : ex.dt, ex.s);
    }));
  }
  TRY(ex.linear(t.attn_out, att.p, C, x.H, x.W, h.p, C, {nullptr, h.p}));      // h = to_out(att) + h  (in place on h)
  if (kv_ctx) {
    // h = to_out(attn2(norm2(h), ctx)) + h: norm2 folded into to_q (one statistics pass over h), the cross-attention core on the
    // context's K|V, to_out in place on h.  (The fused 320-channel entry and the fp8 path stay attn1-only.)
    float* st2 = (float*)ws->scratch((size_t)M * 2 * sizeof(float));
    TRY(ex.rowstats(h, 1e-5f, st2));
    Act q2 = ex.new_act(C, x.H, x.W, false);
    TRY(ex.linear(t.q2, h.p, C, x.H, x.W, q2.p, C, {st2}));
    Act a2 = ex.new_act(C, x.H, x.W, false);
    TRY(ex.launch("launch_attention_cross failed", 1, 4.0 * ex.B * (double)N * S * C, 2.0 * M * C * es,
                  [&] { return "cross N=" + std::to_string(N) + " S=" + std::to_string(S) + " C=" + std::to_string(C); },
                  [&] { return launch_attention_cross(q2.p, kv_ctx, a2.p, ex.B, N, S, C, 8, ex.x3 ? 2 : ex.dt, ex.s); }));
    TRY(ex.linear(t.out2, a2.p, C, x.H, x.W, h.p, C, {nullptr, h.p}));
  }
  if (t.mlp_stream && mlp_fused_ok(C, ex.dt)) {
    // 320-channel level: norm3 -> GEGLU -> ff.net.2 (+h) [-> proj_out (+x)] in one row-local launch (tfuse.hip); the [M, 4C]
    // hidden tensor and the statistics pass never exist
    const bool proj = mlp_fused_proj();
    if (proj) *out = ex.new_act(C, x.H, x.W, true);
    TRY(ex.launch("launch_mlp_fused failed", 0, 2.0 * M * (8.0 * C * C + 4.0 * C * C + (proj ? 1.0 * C * C : 0.0)),
                  (double)M * C * es * (proj ? 3.0 : 2.0) + (double)mlp_fused_stream_bytes(C),
                  [&] { return "M=" + std::to_string(M) + " mlp_fused C=" + std::to_string(C) + " proj=" + std::to_string((int)proj); }, [&] {
                    return launch_mlp_fused(h.p, proj ? out->p : h.p, x.p, t.mlp_stream, t.ff1.bias, t.ff2.bias, t.proj_out.bias,
                                            igemm_zero_page(), M, C, 1e-5f, proj ? 1 : 0, N, ex.s);
                  }));
    if (!proj) TRY(ex.conv(t.proj_out, h, out, {.resid = &x}));
    ws->reset(m);
    return 0;
  }
  float* stats = (float*)ws->scratch((size_t)M * 2 * sizeof(float));
  TRY(ex.rowstats(h, 1e-5f, stats));          // norm3, folded into the GEGLU GEMM the same way
  ff = ex.new_act(4 * C, x.H, x.W, false);
  TRY(ex.linear(t.ff1, h.p, C, x.H, x.W, ff.p, 4 * C, {stats, nullptr, EPI_GEGLU}));
  if (t.ffp.w && g_ffp_mode) {
    // out = proj_out(h + ff.net.2(g)) + x as one Linear over torch.cat([g, h], -1) (TransformerW::ffp)
    TRY(ex.conv(t.ffp, ff, out, {.x2 = &h, .resid = &x}));
    ws->reset(m);
    return 0;
  }
  TRY(ex.linear(t.ff2, ff.p, 4 * C, x.H, x.W, h.p, C, {nullptr, h.p}));
  TRY(ex.conv(t.proj_out, h, out, {.resid = &x}));
  ws->reset(m);
  return 0;
}

// The 12 residual tensors of the separate image encoder, in the order of the skip connections: elements of each and of all
struct ImgResidLayout {
  size_t elems[12], off[12], total = 0;      // off: in elements
  ImgResidLayout(int B, int L) {
    int k = 0;
    auto add = [&](int C, int side) { elems[k] = (size_t)B * side * side * C; off[k] = total; total += rup(elems[k], 128); ++k; };
    add(kBlockOut[0], L);
    for (int i = 0; i < 4; ++i) {
      add(kBlockOut[i], L >> i);
      add(kBlockOut[i], L >> i);
      if (i < 3) add(kBlockOut[i], L >> (i + 1));
    }
  }
};
// room for them at (B, L); growth synchronises the device (ldmseg_unet_reserve does it up front)
int img_resid_reserve(ldmseg_unet* u, int B, int L) {
  if (!u->sepenc) return 0;
  const size_t need = ImgResidLayout(B, L).total * esize(u->dt);
  if (need <= u->img_resid_bytes) return 0;
  HIP_TRY(hipDeviceSynchronize());
  if (u->img_resid) (void)hipFree(u->img_resid);
  u->img_resid = nullptr; u->img_resid_bytes = 0;
  if (hipMalloc(&u->img_resid, need) != hipSuccess) return fail(LDMSEG_E_OOM, "hipMalloc of the image-encoder residuals failed");
  u->img_resid_bytes = need;
  return 0;
}

// One forward's request: what an entry point or a sampling loop asks of the UNet.  The handle keeps only what outlives a call.
struct UnetCall {
  const float *a = nullptr, *b = nullptr, *c = nullptr;      // up to three fp32 NCHW inputs, channel-concatenated: Ca + Cb + Cc = in_channels
  int Ca = 0, Cb = 0, Cc = 0;
  const int64_t* t_dev = nullptr;      // timestep: device int64 (t_count 1 or B) or, t_dev null, t_host
  int t_count = 1;
  int64_t t_host = 0;
  const int64_t* timg_dev = nullptr; int timg_count = 1; int64_t timg_host = 0;      // timestep_img of a separate-encoder handle, likewise
  int B = 0, L = 0;
  float* out = nullptr;                // [B,4,L,L] fp32
  hipStream_t s = nullptr;
  const float* ctx = nullptr;          // [B, S, ctx_dim] fp32 (cross-attention handles)
  int S = 0, ctx_dim = kCrossDim;
  const float* temb_row = nullptr;     // this step's time_emb_proj row from the loop's table (broadcast over the batch); null: computed here
  const StepTail* tail = nullptr;      // the scheduler step offered to the conv_out launch (tail.hip) ...
  bool tail_done = false;              // ... and whether the forward carried it out
  bool img_keep = false;               // image-encoder residuals computed by this forward stay valid for the forwards after it
};

int check_bl(int B, int L) {
  if (B < 1 || L < 8 || L % 8 != 0) return fail(LDMSEG_E_SHAPE, "L must be a positive multiple of 8, B >= 1");
  return 0;
}
// the one validation of a request's shapes: the passes below trust it
int unet_check(const ldmseg_unet* u, const UnetCall& q) {
  if (q.timg_count != 1 && q.timg_count != q.B) return fail(LDMSEG_E_ARG, "timg_count must be 1 or B");
  TRY(check_bl(q.B, q.L));
  if ((u->sepenc && q.Cc) || q.Ca + q.Cb + q.Cc != u->cfg.in_channels) return fail(LDMSEG_E_SHAPE, "input channel count != in_channels");
  if (q.t_dev && q.t_count != 1 && q.t_count != q.B) return fail(LDMSEG_E_ARG, "t_count must be 1 or B");
  return 0;
}

// The time-embedding MLP, written once: n timesteps -> sinusoid -> linear_1 -> SiLU -> linear_2 -> all time_emb_proj(SiLU(.)) of one
// table (pw, pb: `total` columns) -> rows [n][total], in chunks of 64 rows.
struct TimeBufs { float *sinus, *e1, *emb, *rows; };     // [n][320], [n][kTimeDim] twice, [n][total]
int time_mlp(const ldmseg_unet* u, const int64_t* t_dev, int t_count, int64_t t_host, int n, const TimeBufs& tb, const float* pw,
             const float* pb, int total, hipStream_t s) {
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int r = n - i0 < 64 ? n - i0 : 64;
    float *si = tb.sinus + (size_t)i0 * 320, *e1 = tb.e1 + (size_t)i0 * kTimeDim, *em = tb.emb + (size_t)i0 * kTimeDim;
    int rc = launch_time_embed(t_dev ? t_dev + i0 : nullptr, t_dev && t_count > 1 ? r : t_count, t_host, r, si, s);
    if (!rc) rc = launch_small_linear(si, u->te1_w, u->te1_b, e1, r, 320, kTimeDim, 0, 1, s);
    if (!rc) rc = launch_small_linear(e1, u->te2_w, u->te2_b, em, r, kTimeDim, kTimeDim, 0, 0, s);
    if (!rc) rc = launch_small_linear(em, pw, pb, tb.rows + (size_t)i0 * total, r, kTimeDim, total, 1, 0, s);
    if (rc) return rc;      // (a launcher code: the callers name it)
  }
  return 0;
}

// The rows of one pass, in its workspace: a scalar timestep (timestep.expand(B), unet.py:302-303) gives every image the same
// embedding, so the MLP runs for one row that is broadcast (stride 0) instead of B identical rows.  given: the loop's row instead.
struct TimeRows { const float* p = nullptr; int stride = 0; };
int pass_time_rows(Exec& ex, const ldmseg_unet* u, const int64_t* t_dev, int t_count, int64_t t_host, const float* pw, const float* pb,
                   int total, const float* given, TimeRows* out) {
  Workspace* ws = ex.ws;
  const bool per_sample = t_dev != nullptr && t_count > 1;
  TimeBufs tb;
  tb.sinus = (float*)ws->persist((size_t)ex.B * 320 * sizeof(float));
  tb.e1 = (float*)ws->persist((size_t)ex.B * kTimeDim * sizeof(float));
  tb.emb = (float*)ws->persist((size_t)ex.B * kTimeDim * sizeof(float));
  tb.rows = (float*)ws->persist((size_t)ex.B * total * sizeof(float));
  if (given && !ex.dry()) { *out = {given, 0}; return 0; }
  *out = {tb.rows, per_sample ? total : 0};
  return ex.launch("time embedding failed", 4, 0, 0, no_label, [&] { return time_mlp(u, t_dev, t_count, t_host, per_sample ? ex.B : 1, tb, pw, pb, total, ex.s); });
}

// The down path, written once: resnet [-> transformer] twice per level, a stride-2 conv between levels.  made(h, level) sees every
// tensor it produces (12 with the caller's conv_in output).  kv: the six transformers' context K|V (null: no attn2).
template <typename Made>
int walk_down(Exec& ex, const ResnetW (&res)[4][2], const TransformerW (&attn)[3][2], const ConvW (&down)[3], const TimeRows& te,
              const void* const* kv, int S, Act* h, Made&& made) {
  for (int i = 0; i < 4; ++i) {
    for (int j = 0; j < 2; ++j) {
      Act o;
      TRY(run_resnet(ex, res[i][j], *h, nullptr, te.p, te.stride, &o));
      *h = o;
      if (i < 3) {
        TRY(run_transformer(ex, attn[i][j], *h, &o, kv[2 * i + j], S));
        *h = o;
      }
      TRY(made(*h, i));
    }
    if (i < 3) {
      Act o;
      TRY(ex.conv(down[i], *h, &o, {.stride = 2}));
      *h = o;
      TRY(made(*h, i));
    }
  }
  return 0;
}

Exec unet_exec(ldmseg_unet* u, int B, hipStream_t s, bool dry, size_t scratch_base) {
  Exec ex = make_exec(*u, B, s, dry, scratch_base);
  ex.attn_fp8_min_tokens = u->attn_fp8_min_tokens;
  ex.gn_poll_us = u->gn_backoff_calls > 0 ? 2 : -1;
  return ex;
}

// The image branch of a separate-encoder handle as a workspace pass of its own (unet.py:309-351): emb(timestep_img), conv_in_img on
// the RGB half of the packed input, down_blocks_additional, adaptor_layers - its 12 outputs land in u->img_resid.  (a | b: the
// 8-channel input or its two halves, as unet_forward_impl takes them; the segmentation half meets zero weights.)
int unet_img_branch_impl(ldmseg_unet* u, const UnetCall& q, bool dry, size_t scratch_base) {
  const int B = q.B, L = q.L, dt = u->dt;
  hipStream_t s = q.s;
  Workspace* ws = &u->ws;
  Exec ex = unet_exec(u, B, s, dry, scratch_base);
  const ImgResidLayout lay(B, L);
  if (!dry && lay.total * esize(dt) > u->img_resid_bytes) return fail(LDMSEG_E_OOM, "image-encoder residual buffer too small");
  auto resid = [&](int k) { return (void*)((char*)u->img_resid + lay.off[k] * esize(dt)); };
  TimeRows te;
  TRY(pass_time_rows(ex, u, q.timg_dev, q.timg_count, q.timg_host, u->tproj_img_w, u->tproj_img_b, u->temb_img_total, nullptr, &te));

  Act xin = ex.new_act(bke(dt), L, L, true);
  TRY(ex.launch("launch_pack_concat3 failed", 4, 0, 0, no_label, [&] { return launch_pack_concat3(q.a, q.Ca, q.b, q.Cb, nullptr, 0, xin.p, B, L * L, bke(dt), dt, s); }));
  int k = 0;
  // residual k <- h (the first: conv_in_img's output as it is) or adaptor_layers[block](h)
  auto emit = [&](const Act& h, int block) -> int {
    if (block >= 0 && u->adaptor) {
      const size_t m = ws->mark();
      Act o;
      TRY(ex.conv(u->adapt[block], h, &o, {.persist = false, .dst = resid(k)}));
      ws->reset(m);
    } else if (!dry) {
      TRY(ex.ws_ok());
      HIP_TRY(hipMemcpyAsync(resid(k), h.p, lay.elems[k] * esize(dt), hipMemcpyDeviceToDevice, s));
    }
    ++k;
    return 0;
  };
  Act h;
  TRY(ex.conv(u->conv_in_img, xin, &h));
  TRY(emit(h, -1));
  const void* const no_kv[6] = {};
  return walk_down(ex, u->img_res, u->img_attn, u->img_conv, te, no_kv, 0, &h, emit);
}

// dry = true only measures the workspace
int unet_forward_impl(ldmseg_unet* u, UnetCall& q, bool dry, size_t scratch_base) {
  const int B = q.B, L = q.L, dt = u->dt;
  hipStream_t s = q.s;
  Workspace* ws = &u->ws;
  Exec ex = unet_exec(u, B, s, dry, scratch_base);

  // --- time embedding: sinusoid -> MLP -> every resnet's time_emb_proj(SiLU(emb)), or the loop's row (read-only) ---
  TimeRows te;
  TRY(pass_time_rows(ex, u, q.t_dev, q.t_count, q.t_host, u->tproj_w, u->tproj_b, u->temb_total, q.temb_row, &te));

  // --- cross-attention handles: K|V of the context for all 16 transformers (persist: the same offsets in every forward of a
  // plan, so the guided sampling loop computes them in its first step only) ---
  const void* kv_ctx[kTransformers] = {};
  const int S = u->cfg.cross_attention ? u->ctx_S : 0;
  if (u->cfg.cross_attention) {
    if (!dry && !q.ctx) return fail(LDMSEG_E_ARG, "cross-attention handle: no context");
    const TransformerW* tw[kTransformers];
    int nt = 0;
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 2; ++j) tw[nt++] = &u->down_attn[i][j];
    tw[nt++] = &u->mid_attn;
    for (int i = 1; i < 4; ++i) for (int j = 0; j < 3; ++j) tw[nt++] = &u->up_attn[i][j];
    for (int k = 0; k < kTransformers; ++k) kv_ctx[k] = ws->persist((size_t)B * S * 2 * tw[k]->C * esize(dt));
    const bool reuse = !dry && u->ctx_kv_ready && u->ctx_kv_base == (const void*)ws->base;
    if (!reuse) {
      const size_t m0 = ws->mark();
      Act c = ex.new_act(u->ctx_dim, S, 1, false);          // [B*S, ctx_dim] in the compute dtype
      if (dt == DT_F32) {
        c.p = const_cast<float*>(q.ctx);
      } else if (!dry) {
        TRY(ex.ws_ok());
        TRY(launch_rows_to_dtype(q.ctx, c.p, (size_t)B * S * u->ctx_dim, dt, s));
      }
      if (u->ctx_dim == kHidProjIn) {
        Act c2;
        TRY(ex.conv(u->hid_proj, c, &c2, {.persist = false}));    // encoder_hid_proj (unet.py:319-320)
        c = c2;
      }
      for (int k = 0; k < kTransformers; ++k) {
        const ConvW& w = tw[k]->kv2;
        TRY(ex.linear(w, c.p, kCrossDim, S, 1, const_cast<void*>(kv_ctx[k]), w.n_valid));
      }
      ws->reset(m0);
      if (!dry) u->ctx_kv_base = ws->base;
    }
  }

  // --- conv_in on the channel-concatenated fp32 NCHW input ---
  Act xin = ex.new_act(bke(dt), L, L, true);
  // (a re-plan or a workspace reallocation between two steps moves xin: the pointer the tail wrote to must be this one)
  const bool xin_kept = !dry && u->xin_ready && u->xin_ptr == xin.p;
  if (!dry) { u->xin_ready = false; u->xin_ptr = nullptr; }
  if (!xin_kept)      // (kept: the previous step's tail already wrote [latents | rgb | cond] here, tail.hip)
    TRY(ex.launch("launch_pack_concat3 failed", 4, 0, 0, no_label, [&] { return launch_pack_concat3(q.a, q.Ca, q.b, q.Cb, q.c, q.Cc, xin.p, B, L * L, bke(dt), dt, s); }));
  Act h;
  TRY(ex.conv(u->conv_in, xin, &h));
  std::vector<Act> skips{h};
  TRY(walk_down(ex, u->down_res, u->down_attn, u->down_conv, te, kv_ctx, S, &h, [&](const Act& t, int) { skips.push_back(t); return 0; }));
  if (u->sepenc) {
    // skip k += residual k of the image branch (unet.py:375-385), one launch.  The last skip is also the mid block's input, which
    // stays un-summed: its sum goes to a tensor of its own; the other 11 are summed in place.
    const ImgResidLayout lay(B, L);
    Act last = ex.new_act(skips[11].C, skips[11].H, skips[11].W, true);
    SkipAddSeg segs[12];
    for (int k = 0; k < 12; ++k) {
      if ((size_t)B * skips[k].H * skips[k].W * skips[k].C != lay.elems[k]) return fail(LDMSEG_E_SHAPE, "skip / residual shape mismatch");
      segs[k].dst = k == 11 ? last.p : skips[k].p;
      segs[k].a = skips[k].p;
      segs[k].b = (const char*)u->img_resid + lay.off[k] * esize(dt);
      segs[k].elems = (long long)lay.elems[k];
    }
    skips[11] = last;
    if (!dry && lay.total * esize(dt) > u->img_resid_bytes) return fail(LDMSEG_E_OOM, "image-encoder residual buffer too small");
    TRY(ex.launch("launch_skip_add failed", 4, 0, 3.0 * lay.total * esize(dt), [] { return std::string("skip_add"); }, [&] { return launch_skip_add(segs, 12, dt, s); }));
  }
  {
    Act o;
    TRY(run_resnet(ex, u->mid_res[0], h, nullptr, te.p, te.stride, &o)); h = o;
    TRY(run_transformer(ex, u->mid_attn, h, &o, kv_ctx[6], S)); h = o;
    TRY(run_resnet(ex, u->mid_res[1], h, nullptr, te.p, te.stride, &o)); h = o;
  }
  for (int i = 0; i < 4; ++i) {
    for (int j = 0; j < 3; ++j) {
      Act sk = skips.back();
      skips.pop_back();
      Act o;
      TRY(run_resnet(ex, u->up_res[i][j], h, &sk, te.p, te.stride, &o));   // torch.cat([hidden, skip], 1)
      h = o;
      if (i > 0) {
        TRY(run_transformer(ex, u->up_attn[i][j], h, &o, kv_ctx[7 + 3 * (i - 1) + j], S));
        h = o;
      }
    }
    if (i < 3) {
      Act o;
      TRY(ex.conv(u->up_conv[i], h, &o, {.up = 1}));  // nearest x2 folded in
      h = o;
    }
  }
  // --- conv_norm_out -> SiLU -> conv_out, written straight to fp32 NCHW ---
  {
    const size_t m = ws->mark();
    Act n;
    TRY(ex.groupnorm(u->norm_out, h, nullptr, 1e-5f, 1, &n));
    if (conv_out_tail_ok(n.C, L, L, dt)) {
      // bf16: conv_out as a halo-resident stencil and - inside ldmseg_sample_loop - the rest of the step in its epilogue
      StepTail t;
      if (q.tail && step_tail_fused() && !dry) {
        t = *q.tail;
        t.xin_next = t.last ? nullptr : xin.p;
        t.eps_out = nullptr;
      } else {
        t.eps_out = q.out;
      }
      t.x = n.p; t.w = u->conv_out.w; t.bias = u->conv_out.bias; t.zeros = igemm_zero_page();
      t.B = B; t.H = L; t.W = L;
      TRY(ex.launch("launch_conv_out_tail failed", 0, 2.0 * B * L * L * 4 * 9 * n.C, (double)B * L * L * n.C * esize(dt),
                    [&] { return "M=" + std::to_string(B * L * L) + " conv_out_tail ddim=" + std::to_string(t.ddim); },
                    [&] { return launch_conv_out_tail(t, s); }));
      if (!dry && t.ddim) { q.tail_done = true; u->xin_ready = t.xin_next != nullptr; u->xin_ptr = t.xin_next; }
    } else {
      IgemmParams p;
      p.src0 = n.p; p.C0 = n.C; p.B = B; p.Hi = p.Ho = L; p.Wi = p.Wo = L;
      p.taps = 9; p.M = B * L * L; p.N = u->conv_out.N; p.n_valid = 4;
      p.W = u->conv_out.w; p.bias = u->conv_out.bias; p.out = q.out; p.epi = EPI_NCHW_F32;
      TRY(ex.igemm(p));
    }
    ws->reset(m);
  }
  return 0;
}

// One forward = the image branch (separate-encoder handles whose residuals are not standing, see ldmseg_sample_loop), then the UNet
// itself.  Both are passes over the same workspace from its start - the branch leaves its results in u->img_resid - so the offsets
// of the UNet's pass are those of a plain handle whether the branch ran or not; a dry run measures both and keeps the larger peaks.
int unet_forward_passes(ldmseg_unet* u, UnetCall& q, bool dry, size_t scratch_base) {
  size_t pp = 0, sp = 0;
  if (u->sepenc && (dry || !u->img_ready)) {
    TRY(unet_img_branch_impl(u, q, dry, scratch_base));
    pp = u->ws.persist_peak; sp = u->ws.scratch_peak;
    if (!dry) {
      u->img_ready = q.img_keep;
      u->xin_ready = false; u->xin_ptr = nullptr;      // (the pass went over the place where a step tail left the next input)
    }
  }
  TRY(unet_forward_impl(u, q, dry, scratch_base));
  if (dry) {
    u->ws.persist_peak = std::max(u->ws.persist_peak, pp);
    u->ws.scratch_peak = std::max(u->ws.scratch_peak, sp);
  }
  return 0;
}

// a request, checked here and nowhere below, on a workspace planned for its shape
int unet_run(ldmseg_unet* u, UnetCall& q) {
  TRY(unet_check(u, q));
  if (u->cfg.cross_attention) { u->ctx_S = q.S; u->ctx_dim = q.ctx_dim; }
  TRY(img_resid_reserve(u, q.B, q.L));      // no-op after ldmseg_unet_reserve or a previous call at this size
  const PlanKey key{q.B, q.L, u->ctx_S, u->ctx_dim};
  const void* before = u->ws_mem;
  const size_t cap_before = u->ws_cap;
  return plan_and_run(*u, &key, [&](bool dry, size_t scratch_base) {
    // (the workspace moved or grew: a new arena may reuse the old address, so the tail's hand-over is void either way)
    if (!dry && (u->ws_mem != before || u->ws_cap != cap_before)) { u->xin_ready = false; u->xin_ptr = nullptr; }
    return unet_forward_passes(u, q, dry, scratch_base);
  });
}

// what a call may leave standing in the handle for its own later forwards, gone when the call returns (also on an error)
struct CallScrub {
  ldmseg_unet* u;
  ~CallScrub() { u->xin_ready = false; u->xin_ptr = nullptr; u->img_ready = false; u->ctx_kv_ready = false; u->ctx_kv_base = nullptr; }
};

// what the three context-free forward entries share (args: the entry's pointers are there; q.Ca 0: one input of in_channels channels)
int plain_forward(ldmseg_unet* h, bool args, UnetCall q) {
  g_err.clear();
  if (!h || !args) return fail(LDMSEG_E_ARG, "null argument");
  if (h->cfg.cross_attention) return fail(LDMSEG_E_ARG, "cross-attention handle: the context goes through ldmseg_unet_forward_ctx");
  if (!q.Ca) q.Ca = h->cfg.in_channels;
  DeviceGuard dg(h->cfg.device);
  return unet_run(h, q);
}
// the context argument of the cross-attention entry points
int check_ctx(const ldmseg_unet* h, const float* ctx, int S, int ctx_dim) {
  if (!h->cfg.cross_attention) return fail(LDMSEG_E_ARG, "handle built without cross-attention: no context");
  if (!ctx) return fail(LDMSEG_E_ARG, "null context");
  if (S < 1 || S > 4096) return fail(LDMSEG_E_ARG, "context length S must be in [1, 4096]");
  if (ctx_dim != kCrossDim && !(ctx_dim == kHidProjIn && h->hid_proj.w))
    return fail(LDMSEG_E_ARG, "ctx_dim must be 768 (or 1024 on a handle holding encoder_hid_proj)");
  return 0;
}

// room for the time-embedding rows of `n_steps` steps (at least 64: 6 MB, so that a short warm-up call followed by a longer
// run does not re-allocate); ldmseg_unet_reserve sizes it up front
int temb_reserve(ldmseg_unet* h, int n_steps) {
  if (h->temb_cap >= n_steps) return 0;
  const size_t per = sizeof(int64_t) + (320 + 2 * (size_t)kTimeDim + h->temb_total) * sizeof(float);
  int cap = 64;
  while (cap < n_steps) cap *= 2;
  HIP_TRY(hipDeviceSynchronize());
  if (h->temb_buf) (void)hipFree(h->temb_buf);
  h->temb_buf = nullptr; h->temb_cap = 0;
  HIP_TRY(hipMalloc(&h->temb_buf, per * cap));
  h->temb_cap = cap;
  return 0;
}
// (re)allocate the sampler's eps / self-condition buffers; growth synchronises the device
int loop_reserve(ldmseg_unet* h, size_t n) {
  if (h->loop_elems >= n) return 0;
  HIP_TRY(hipDeviceSynchronize());
  if (h->cond) (void)hipFree(h->cond);
  if (h->eps) (void)hipFree(h->eps);
  h->cond = h->eps = nullptr;
  h->loop_elems = 0;
  HIP_TRY(hipMalloc((void**)&h->cond, n * sizeof(float)));
  HIP_TRY(hipMalloc((void**)&h->eps, n * sizeof(float)));
  h->loop_elems = n;
  return 0;
}

// the refusals both sampling loops share, in the two runs in which they stand between a loop's own
int loop_steps_ok(const ldmseg_sample_cfg* cfg, int B, int L) {
  if (cfg->n_steps < 1) return fail(LDMSEG_E_ARG, "n_steps must be >= 1");
  TRY(check_bl(B, L));
  return cfg->prediction_type < 0 || cfg->prediction_type > 2 ? fail(LDMSEG_E_ARG, "unknown prediction_type") : 0;
}
int loop_timesteps_ok(const ldmseg_sample_cfg* cfg) {
  for (int i = 0; i < cfg->n_steps; ++i)
    if (cfg->timesteps[i] < 0) return fail(LDMSEG_E_ARG, "negative timestep");
  return 0;
}
const char* const kSelfCondMismatch = "self_condition needs the 12-channel conv_in (and vice versa)";

// The frame of both sampling loops: the reserves, the table of time-embedding rows, the GroupNorm back-off, and around each step its
// DdimCoef, the all_latents copy and at the end the diagnostic copy.  step(i, q, dc, last) is the loop's own: q carries the step's
// timestep, time-embedding row, stream, L, the self-condition input and eps as the output.  images: how many the forwards of a step
// run for each of the B (eps holds them all).
template <typename Step>
int sample_steps(ldmseg_unet* h, const ldmseg_sample_cfg* cfg, float* latents, int B, int L, int images, float* all_latents, hipStream_t s,
                 Step&& step) {
  const size_t n = (size_t)B * 4 * L * L;
  const bool selfc = cfg->self_condition != 0;
  TRY(loop_reserve(h, (size_t)images * n));      // no-op after ldmseg_unet_reserve or a previous call at this size
  if (selfc) HIP_TRY(hipMemsetAsync(h->cond, 0, n * sizeof(float), s));   // condition = zeros_like(rgb_latents)
  // the time-embedding rows of every step: rows[i] = time_emb_proj_all(silu(MLP(sinusoid(timesteps[i]))))
  TRY(temb_reserve(h, cfg->n_steps));
  int64_t* ts = (int64_t*)h->temb_buf;
  TimeBufs tb;
  tb.sinus = (float*)(ts + h->temb_cap);
  tb.e1 = tb.sinus + (size_t)h->temb_cap * 320;
  tb.emb = tb.e1 + (size_t)h->temb_cap * kTimeDim;
  tb.rows = tb.emb + (size_t)h->temb_cap * kTimeDim;
  HIP_TRY(hipMemcpyAsync(ts, cfg->timesteps, (size_t)cfg->n_steps * sizeof(int64_t), hipMemcpyHostToDevice, s));
  TRY(launch_code(time_mlp(h, ts, cfg->n_steps, 0, cfg->n_steps, tb, h->tproj_w, h->tproj_b, h->temb_total, s), "time embedding failed"));
  if (h->gn_sync) {                  // cooperative GroupNorm back-off: did the previous calls' norms miss their partners?
    if (!h->gn_diag_host) {
      HIP_TRY(hipHostMalloc((void**)&h->gn_diag_host, sizeof(unsigned long long)));
      *h->gn_diag_host = 0;
    }
    const unsigned long long cur = *(volatile unsigned long long*)h->gn_diag_host;     // whatever the last finished copy left
    // (only launches under the full bound count - norm.hip - so the eight short-bound calls decay unconditionally and the
    // ninth probes the full bound again)
    if (cur >= h->gn_diag_seen + 256) h->gn_backoff_calls = 8;
    else if (h->gn_backoff_calls > 0) --h->gn_backoff_calls;
    h->gn_diag_seen = cur;
  }
  CallScrub scrub{h};
  h->img_ready = false;
  for (int i = 0; i < cfg->n_steps; ++i) {
    const float* c = cfg->coef + 4 * i;
    const DdimCoef dc{c[0], c[1], c[2], c[3], cfg->prediction_type, cfg->clip_sample, cfg->clip_sample_range, 0};
    UnetCall q;
    q.Ca = q.Cb = 4;
    if (selfc) { q.c = h->cond; q.Cc = 4; }
    q.t_host = cfg->timesteps[i];
    q.B = images * B; q.L = L; q.out = h->eps; q.s = s;
    q.temb_row = tb.rows + (size_t)i * h->temb_total;
    TRY(step(i, q, dc, i == cfg->n_steps - 1));
    if (all_latents)
      HIP_TRY(hipMemcpyAsync(all_latents + (size_t)i * n, latents, n * sizeof(float), hipMemcpyDeviceToDevice, s));
  }
  if (h->gn_sync && h->gn_diag_host)
    HIP_TRY(hipMemcpyAsync(h->gn_diag_host, gn_sync_diag_ptr(h->gn_sync), sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  return 0;
}

}  // namespace

// =================================================================== C ABI
extern "C" {

int ldmseg_unet_create(const ldmseg_unet_cfg* cfg, int n_weights, const char* const* names,
                       const void* const* dev_ptrs, const int64_t* numels, ldmseg_unet** out) {
  bool sepenc = false;
  for (int i = 0; names && i < n_weights; ++i) sepenc = sepenc || (names[i] && std::strcmp(names[i], "conv_in_img.weight") == 0);
  auto check = [sepenc](const ldmseg_unet_cfg& c) {
    if (c.cross_attention != 0 && c.cross_attention != 1) return fail(LDMSEG_E_ARG, "cross_attention must be 0 or 1");
    if (c.in_channels != 4 && c.in_channels != 8 && c.in_channels != 12) return fail(LDMSEG_E_ARG, "in_channels must be 4, 8 or 12");
    // (before any device work: a state dict with conv_in_img.* is a separate-encoder UNet, unet.py:42-63)
    if (sepenc && c.cross_attention) return fail(LDMSEG_E_ARG, "separate image encoder (conv_in_img.*) with cross_attention is not supported");
    if (sepenc && c.in_channels != 8) return fail(LDMSEG_E_ARG, "separate image encoder (conv_in_img.*) needs in_channels 8");
    return 0;
  };
  return create_handle(cfg, n_weights, names, dev_ptrs, numels, check, unet_build, true, out);
}

LDMSEG_HANDLE_ABI(ldmseg_unet)

size_t ldmseg_unet_workspace_bytes(const ldmseg_unet* h, int B, int L) {
  if (!h) return 0;
  ldmseg_unet* u = const_cast<ldmseg_unet*>(h);
  DeviceGuard dg(u->cfg.device);
  UnetCall q{.Ca = u->cfg.in_channels, .B = B, .L = L};      // shapes only: a request that measures
  if (unet_check(u, q) != 0 || unet_forward_passes(u, q, true, 0) != 0) return 0;
  return rup(u->ws.persist_peak, 4096) + rup(u->ws.scratch_peak, 4096);
}

int ldmseg_unet_forward(ldmseg_unet* h, const float* x, const int64_t* t_dev, int t_count, int64_t t_host, int B, int L,
                        float* out, void* stream) {
  return plain_forward(h, x && out, {.a = x, .t_dev = t_dev, .t_count = t_count, .t_host = t_host, .B = B, .L = L, .out = out, .s = (hipStream_t)stream});
}

int ldmseg_unet_forward_parts(ldmseg_unet* h, const float* latents, const float* rgb_latents, const float* cond,
                              const int64_t* t_dev, int t_count, int64_t t_host, int B, int L, float* out, void* stream) {
  return plain_forward(h, latents && rgb_latents && out, {.a = latents, .b = rgb_latents, .c = cond, .Ca = 4, .Cb = 4, .Cc = cond ? 4 : 0, .t_dev = t_dev,
                                                          .t_count = t_count, .t_host = t_host, .B = B, .L = L, .out = out, .s = (hipStream_t)stream});
}

int ldmseg_unet_forward_img(ldmseg_unet* h, const float* x, const int64_t* t_dev, int t_count, int64_t t_host,
                            const int64_t* timg_dev, int timg_count, int64_t timg_host, int B, int L, float* out, void* stream) {
  return plain_forward(h, x && out, {.a = x, .t_dev = t_dev, .t_count = t_count, .t_host = t_host, .timg_dev = timg_dev, .timg_count = timg_count, .timg_host = timg_host, .B = B, .L = L,
                                     .out = out, .s = (hipStream_t)stream});
}

int ldmseg_unet_forward_ctx(ldmseg_unet* h, const float* x, const int64_t* t_dev, int t_count, int64_t t_host, int B, int L,
                            const float* ctx, int S, int ctx_dim, float* out, void* stream) {
  g_err.clear();
  if (!h || !x || !out) return fail(LDMSEG_E_ARG, "null argument");
  TRY(check_ctx(h, ctx, S, ctx_dim));
  CallScrub scrub{h};
  DeviceGuard dg(h->cfg.device);
  UnetCall q{.a = x, .Ca = h->cfg.in_channels, .t_dev = t_dev, .t_count = t_count, .t_host = t_host, .B = B, .L = L, .out = out, .s = (hipStream_t)stream,
             .ctx = ctx, .S = S, .ctx_dim = ctx_dim};
  return unet_run(h, q);
}

int ldmseg_unet_set_attention_fp8(ldmseg_unet* h, int min_tokens) {
  g_err.clear();
  if (!h || min_tokens < 0) return fail(LDMSEG_E_ARG, "bad argument");
  if (min_tokens > 0 && h->dt != DT_BF16) return fail(LDMSEG_E_ARG, "the fp8 attention path belongs to the bf16 perf mode");
  h->attn_fp8_min_tokens = min_tokens;
  h->plan_valid = false;              // the workspace plan depends on it
  return 0;
}

int ldmseg_unet_reserve(ldmseg_unet* h, int B, int L) {
  g_err.clear();
  if (!h) return fail(LDMSEG_E_ARG, "null argument");
  DeviceGuard dg(h->cfg.device);
  UnetCall q{.Ca = h->cfg.in_channels, .B = B, .L = L};      // shapes only: a request that reserves
  TRY(unet_check(h, q));
  const PlanKey key{B, L, h->ctx_S, h->ctx_dim};
  TRY(plan_workspace(*h, &key, [&](bool dry, size_t scratch_base) { return unet_forward_passes(h, q, dry, scratch_base); }));
  TRY(img_resid_reserve(h, B, L));
  TRY(loop_reserve(h, (size_t)B * 4 * L * L));
  TRY(temb_reserve(h, 64));
  TRY(igemm_warm());
  return 0;
}

// Test support (include/ldmseg_hip_ops.h): the handle's own time_mlp for n host timesteps on one of its time_emb_proj tables, the way
// the sampling loops call it (timesteps on the device, one per row), on scratch memory of this call.  Waits for the stream.
int ldmseg_unet_time_rows(ldmseg_unet* h, const int64_t* timesteps_host, int n, int table, float* rows_dev, int* total_out,
                          void* stream) {
  g_err.clear();
  if (!h || !timesteps_host || !total_out) return fail(LDMSEG_E_SHAPE, "null argument");
  if (n < 1) return fail(LDMSEG_E_SHAPE, "n must be >= 1");
  for (int i = 0; i < n; ++i)
    if (timesteps_host[i] < 0) return fail(LDMSEG_E_SHAPE, "negative timestep");
  if (table != 0 && !(table == 1 && h->sepenc)) return fail(LDMSEG_E_SHAPE, "table must be 0, or 1 on a separate-encoder handle");
  const float* pw = table ? h->tproj_img_w : h->tproj_w;
  const float* pb = table ? h->tproj_img_b : h->tproj_b;
  const int total = table ? h->temb_img_total : h->temb_total;
  *total_out = total;
  if (!rows_dev) return 0;
  DeviceGuard dg(h->cfg.device);
  hipStream_t s = (hipStream_t)stream;
  struct Scratch {
    void* p = nullptr;
    ~Scratch() { if (p) (void)hipFree(p); }
  } mem;
  HIP_TRY(hipMalloc(&mem.p, (size_t)n * (sizeof(int64_t) + (320 + 2 * (size_t)kTimeDim) * sizeof(float))));
  int64_t* ts = (int64_t*)mem.p;
  TimeBufs tb;
  tb.sinus = (float*)(ts + n);
  tb.e1 = tb.sinus + (size_t)n * 320;
  tb.emb = tb.e1 + (size_t)n * kTimeDim;
  tb.rows = rows_dev;
  HIP_TRY(hipMemcpyAsync(ts, timesteps_host, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, s));
  const int rc = time_mlp(h, ts, n, 0, n, tb, pw, pb, total, s);
  HIP_TRY(hipStreamSynchronize(s));      // (before the scratch goes, also after a failed launch)
  return rc ? launch_code(rc, "time embedding failed") : 0;
}

int ldmseg_sample_loop(ldmseg_unet* h, const ldmseg_sample_cfg* cfg, float* latents, const float* rgb_latents, int B, int L,
                       float* all_latents, void* stream) {
  g_err.clear();
  if (!h || !cfg || !latents || !rgb_latents || !cfg->timesteps || !cfg->coef) return fail(LDMSEG_E_ARG, "null argument");
  if (h->cfg.cross_attention) return fail(LDMSEG_E_ARG, "cross-attention handle: sample with ldmseg_sample_loop_guided");
  TRY(loop_steps_ok(cfg, B, L));
  TRY(loop_timesteps_ok(cfg));
  const bool selfc = cfg->self_condition != 0, inpaint = cfg->known_dev != nullptr;
  if ((h->cfg.in_channels == 12) != selfc) return fail(LDMSEG_E_ARG, kSelfCondMismatch);
  if (inpaint && (!cfg->z0_dev || !cfg->noise_dev || !cfg->paste_coef)) return fail(LDMSEG_E_ARG, "inpainting needs z0, noise and paste_coef");
  DeviceGuard dg(h->cfg.device);
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)B * 4 * L * L;
  // Separate-encoder handles: the image branch reads rgb_latents and timestep_img = 0 only (sample() passes no timestep_img,
  // trainers_ldm_cond.py:1141), so its residuals are the same in every step: step 0's forward computes them and they stand until
  // this call returns (nothing is kept across calls: the caller may change rgb_latents).  Debug key 25: every step computes them.
  const bool img_keep = h->sepenc && !g_sepenc_every_step;
  return sample_steps(h, cfg, latents, B, L, 1, all_latents, s, [&](int i, UnetCall& q, const DdimCoef& dc, bool last) -> int {
    // the scheduler step of this iteration, offered to the forward's conv_out launch (bf16: tail.hip carries it out in its
    // epilogue together with the inpainting paste, the self-condition write and the next step's input pack)
    float* const cond = selfc ? h->cond : nullptr;      // (the frame has reserved it by now)
    StepTail st;
    st.ddim = 1; st.last = last ? 1 : 0; st.c = dc; st.latents = latents; st.cond = cond; st.rgb = rgb_latents;
    if (inpaint) { st.known = cfg->known_dev; st.z0 = cfg->z0_dev; st.noise = cfg->noise_dev; st.sa = cfg->paste_coef[2 * i]; st.sb = cfg->paste_coef[2 * i + 1]; }
    q.a = latents; q.b = rgb_latents; q.tail = &st; q.img_keep = img_keep;
    TRY(unet_run(h, q));
    if (q.tail_done) return 0;
    // condition <- pred_original_sample; latents <- prev_sample (last step: pred_original_sample)
    if (!last) {
      TRY(launch_ddim_step(h->eps, latents, latents, cond, n, dc, s));
    } else {
      TRY(launch_ddim_step(h->eps, latents, nullptr, latents, n, dc, s));
    }
    if (inpaint)
      TRY(launch_inpaint_paste(latents, cfg->z0_dev, cfg->noise_dev, cfg->known_dev, cfg->paste_coef[2 * i],
                               cfg->paste_coef[2 * i + 1], B, 4, L * L, s));
    return 0;
  });
}

int ldmseg_sample_loop_guided(ldmseg_unet* h, const ldmseg_sample_cfg* cfg, float* latents, const float* rgb_latents, int B, int L,
                              const float* ctx, int S, int ctx_dim, int multiplier, float guidance_scale, float* all_latents,
                              void* stream) {
  g_err.clear();
  if (!h || !cfg || !latents || !rgb_latents || !cfg->timesteps || !cfg->coef) return fail(LDMSEG_E_ARG, "null argument");
  TRY(loop_steps_ok(cfg, B, L));
  if (multiplier != 1 && multiplier != 2) return fail(LDMSEG_E_ARG, "multiplier must be 1 or 2");
  TRY(loop_timesteps_ok(cfg));
  const bool selfc = cfg->self_condition != 0;
  // (the reference concatenates a B-row condition with 2B-row tensors there and fails at step 2, trainers_ldm_cond.py:1126-1150)
  if (selfc && multiplier == 2) return fail(LDMSEG_E_ARG, "self_condition with classifier-free guidance (multiplier 2) is not defined");
  if ((h->cfg.in_channels == 12) != selfc) return fail(LDMSEG_E_ARG, kSelfCondMismatch);
  if (cfg->known_dev || cfg->z0_dev || cfg->noise_dev || cfg->paste_coef) return fail(LDMSEG_E_ARG, "inpainting is not combined with guidance");
  if (h->sepenc) return fail(LDMSEG_E_ARG, "separate-encoder handle: no cross-attention, sample with ldmseg_sample_loop");
  TRY(check_ctx(h, ctx, S, ctx_dim));
  DeviceGuard dg(h->cfg.device);
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)B * 4 * L * L;
  float *lat2 = nullptr, *rgb2 = nullptr;
  if (multiplier == 2) {                               // latent_model_input = cat([latents] * 2), rgb likewise (:1122-1133)
    if (h->guide_elems < 4 * n) {
      HIP_TRY(hipDeviceSynchronize());
      if (h->guide_buf) (void)hipFree(h->guide_buf);
      h->guide_buf = nullptr; h->guide_elems = 0;
      HIP_TRY(hipMalloc((void**)&h->guide_buf, 4 * n * sizeof(float)));
      h->guide_elems = 4 * n;
    }
    lat2 = h->guide_buf;
    rgb2 = h->guide_buf + 2 * n;
    for (int k = 0; k < 2; ++k) {
      HIP_TRY(hipMemcpyAsync(lat2 + k * n, latents, n * sizeof(float), hipMemcpyDeviceToDevice, s));
      HIP_TRY(hipMemcpyAsync(rgb2 + k * n, rgb_latents, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
  }
  return sample_steps(h, cfg, latents, B, L, multiplier, all_latents, s, [&](int, UnetCall& q, const DdimCoef& dc, bool last) -> int {
    // the model output of all multiplier * B images lands in h->eps (no fused step tail: the step needs two images' outputs)
    q.a = multiplier == 2 ? lat2 : latents; q.b = multiplier == 2 ? rgb2 : rgb_latents;
    q.ctx = ctx; q.S = S; q.ctx_dim = ctx_dim;
    TRY(unet_run(h, q));
    h->ctx_kv_ready = true;                            // the context does not change across steps
    TRY(launch_guided_step(h->eps, latents, selfc ? h->cond : nullptr, lat2, n, multiplier, guidance_scale, dc, last ? 1 : 0, s));
    return 0;
  });
}

int ldmseg_unet_cf_fallbacks(ldmseg_unet* h, int64_t* count) {
  g_err.clear();
  if (!h || !count) return fail(LDMSEG_E_ARG, "null argument");
  DeviceGuard dg(h->cfg.device);
  unsigned long long n = 0;
  if (h->cf_sync) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(&n, (const unsigned long long*)h->cf_sync + igemm_cf_bytes() / 8 - 1, sizeof n, hipMemcpyDeviceToHost));
  }
  *count = (int64_t)n;
  return 0;
}

int ldmseg_unet_gn_backoff(ldmseg_unet* h, int32_t* calls_left) {
  g_err.clear();
  if (!h || !calls_left) return fail(LDMSEG_E_ARG, "null argument");
  *calls_left = h->gn_backoff_calls;
  return 0;
}

int ldmseg_unet_gn_fallbacks(ldmseg_unet* h, int64_t* count) {
  g_err.clear();
  if (!h || !count) return fail(LDMSEG_E_ARG, "null argument");
  DeviceGuard dg(h->cfg.device);
  const long long n = h->gn_sync ? gn_coop_fallbacks(h->gn_sync) : 0;
  if (n < 0) return fail(LDMSEG_E_HIP, "reading the GroupNorm fallback counter failed");
  *count = n;
  return 0;
}

}  // extern "C"
