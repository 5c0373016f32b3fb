// Which attention kernel a launch runs, on which grid: the forms the attention sources contain (AttnForm; the file named next to
// each form expands the plan's template arguments in its launch_attn_*_plan() - the only place that names them) and the rule that
// picks one (attn_choose).  Plain C++17: no HIP, no state - a function of the launch description and the knobs, so it runs (and
// is tested, tests/test_attn_plan_cpu.py, tools/attn_plan_sweep.cpp) without a device.  DESIGN 3.2 has the rule as a table.
#pragma once
#include <cstddef>
#include <cstdio>
#include <string>

#include "igemm_types.h"   // DType

namespace ldmseg {

enum AttnKind : int { ATTN_KIND_SELF, ATTN_KIND_CAUSAL, ATTN_KIND_FP8, ATTN_KIND_CROSS };
// qkv [B, N, 3C] (cross: q [B, N, C] against S context rows); dtype 0 = fp32, 1 = bf16, 2 = fp32 tensors with split-bf16 products
struct AttnDesc { int kind, B, N, S, C, heads, dtype; };
// variant: debug key 2 (0 = the shipped choice; 1..14 name alternatives kept for A/B measurements and the parity tests);
// mx_mode, mx_variant: debug key 15 (mode 0 = the unscaled fp8 kernel everywhere; variant bit 0 = 8-wave workgroups, bit 1 = the
// direct e4m3 byte in place of exp + convert)
struct AttnKnobs { int variant = 0, mx_mode = 1, mx_variant = 3; };

enum AttnForm : int {
  ATTN_V1,      // attention.hip: attn<T,D,QF>, attn_x3<D,QF>, attn_causal<T,D,QF>, attn_causal_x3<D,QF>
  ATTN_V3,      // attention3.hip: attn3<D,QF,WPS,NST,PIPE,LAZY,NWV>
  ATTN_V4,      // attention4.hip: attn4<d40,NST,LAZY,NWV>
  ATTN_FP8,     // attention_fp8.hip: kv_to_fp8<D,DP>, then attn_fp8<D,QF,WPS,NST>
  ATTN_MX,      // attention_mx.hip: kv_to_mx, then attn_mx<NST,NWV,FEXP>
  ATTN_CROSS,   // attention_cross.hip: attention_cross_kernel<T,D>
};
// Template arguments (D: head dim; QF: 16-row query fragments per wave; WPS: waves per SIMD of the launch bounds; NST: LDS ring
// stages; LAZY: key tiles between two looks at the row maxima; NWV: waves per workgroup; PIPE is always false) and the launch.
// The fp8 forms run a pre-pass first (pre_*: its padded row bytes DP - kv_to_fp8 only - and its launch) into scratch_bytes of
// scratch.  q: the description the plan answers.
struct AttnPlan {
  AttnDesc q{};
  int form = ATTN_V1, D = 0, QF = 1, WPS = 0, NST = 0, LAZY = 1, NWV = 4;
  bool X3 = false, CAUSAL = false, FEXP = false;
  int grid_x = 1, grid_y = 1, grid_z = 1, block = 256;
  int pre_DP = 0, pre_grid_x = 0, pre_grid_y = 1, pre_grid_z = 1, pre_block = 256;
  size_t scratch_bytes = 0;
};

// what the arithmetic below shares with the kernel files (each static_asserts that its own Cfg agrees)
constexpr int kAttnFp8DP40 = 48, kAttnFp8DP80 = 96;       // A8Cfg<D>::DP: fp8 row bytes of the pre-pass, padded to 16
constexpr int kAttnMxTile = 128;                          // keys per tile of the mx form
constexpr int kAttnMxKB = kAttnMxTile * 64, kAttnMxVB = 48 * kAttnMxTile;   // bytes of a tile's K and V^T images
constexpr int kAttnCrossRows = 64;                        // query rows per workgroup of the cross kernel
// query rows per workgroup of the self-attention forms
constexpr int attn_v1_rows(int QF) { return 64 * QF; }            // 4 waves x QF fragments (attn_fp8 as well)
constexpr int attn_v3_rows(int QF, int NWV) { return 16 * NWV * QF; }
constexpr int attn_v4_rows(int NWV) { return 32 * NWV; }          // 32 queries per wave (attn_mx as well)
constexpr int attn_ceil(int a, int b) { return (a + b - 1) / b; }

// attention3.hip's answer to a value of debug key 2 that names one of its instantiations
struct AttnV3Row { int variant, D, QF, WPS, NST, LAZY, NWV; };
constexpr AttnV3Row kAttnV3Variants[] = {
    {1, 40, 1, 4, 3, 1, 4}, {4, 40, 2, 3, 2, 1, 4}, {5, 40, 2, 4, 3, 1, 4},
    {6, 40, 2, 3, 3, 1, 4},                                       // the round-2 kernel: 4 waves, maxima on every tile
    {8, 40, 2, 4, 3, 1, 8},                                       // 8 waves, maxima on every tile
    {9, 40, 2, 4, 3, 4, 8}, {10, 40, 2, 3, 3, 16, 4},
    {1, 80, 1, 3, 2, 1, 4}, {4, 80, 2, 3, 2, 1, 4}, {5, 80, 1, 2, 3, 1, 4},
    {6, 80, 2, 2, 3, 1, 4},                                       // the round-2 kernel
    {8, 80, 1, 4, 3, 16, 8}, {9, 80, 2, 2, 3, 16, 8}, {10, 80, 1, 3, 3, 16, 8},
};

inline void attn_plan_v3(AttnPlan* p, int D, int QF, int WPS, int NST, int LAZY, int NWV) {
  p->form = ATTN_V3;
  p->D = D; p->QF = QF; p->WPS = WPS; p->NST = NST; p->LAZY = LAZY; p->NWV = NWV;
  p->grid_x = attn_ceil(p->q.N, attn_v3_rows(QF, NWV)) * p->q.heads * p->q.B;
  p->block = 64 * NWV;
}
// two ring stages: with three the 8-wave form needs more than the 128 registers four waves per SIMD leave (17-37 spilled, 1.6x
// slower); 2 stages measured as fast as 3 / 4 on the 4-wave form
inline void attn_plan_v4(AttnPlan* p, int LAZY, int NWV) {
  p->form = ATTN_V4;
  p->D = 40; p->QF = 2; p->NST = 2; p->LAZY = LAZY; p->NWV = NWV;
  p->grid_x = attn_ceil(p->q.N, attn_v4_rows(NWV)) * p->q.heads * p->q.B;
  p->block = 64 * NWV;
}
inline int attn_plan_v1(AttnPlan* p, int d, int QF, bool X3, bool CAUSAL) {
  if (d != 40 && d != 64 && d != 80 && d != 160) return -2;
  p->form = ATTN_V1;
  p->D = d; p->QF = d == 160 ? 1 : QF; p->X3 = X3; p->CAUSAL = CAUSAL;
  p->grid_x = attn_ceil(p->q.N, attn_v1_rows(p->QF)) * p->q.heads * p->q.B;
  p->block = 256;
  return 0;
}

// launch_attention: qkv in the description's dtype
inline int attn_choose_self(const AttnKnobs& k, AttnPlan* p) {
  const AttnDesc& q = p->q;
  const int d = q.C / q.heads, v = k.variant;
  // fp32 tensors, split-bf16 products (compute_dtype "bf16x3"): attention.hip, whatever key 2 says
  if (q.dtype == 2) return attn_plan_v1(p, d, q.N >= 256 ? 2 : 1, true, false);
  // bf16 perf mode, head dims 40 / 80: the LDS-DMA + folded-max kernels of attention3.hip / attention4.hip (key 2 = 2, 3 force
  // attention.hip's kernel for A/B measurements)
  if (q.dtype == DT_BF16 && v != 2 && v != 3 && (d == 40 || d == 80)) {
    for (const AttnV3Row& r : kAttnV3Variants)
      if (r.variant == v && r.D == d) { attn_plan_v3(p, r.D, r.QF, r.WPS, r.NST, r.LAZY, r.NWV); return 0; }
    // 8-wave workgroups: 256 query rows share every K / V tile (half the LDS-DMA instructions per score: issuing one parks the
    // wave for 60-185 cycles); short sequences keep the 4-wave form (too few workgroups otherwise)
    const bool big = (long)q.B * q.heads * attn_ceil(q.N, 256) >= 256;
    if (d == 40) {
      // 11..14: attention4.hip, forced form (8 waves lazy / every tile, 4 waves lazy / every tile)
      if (v >= 11 && v <= 14) { attn_plan_v4(p, (v - 11) & 1 ? 1 : 16, v - 11 < 2 ? 8 : 4); return 0; }
      // shipped (0): the 32x32x16 score-block kernel of attention4.hip (round 4: N = 4096 at B = 8 224 -> 196 us, N = 16384 at
      // B = 4 1.67 -> 1.49 ms, N = 1000 15.8 -> 14.1 us); 7 and every other value: attention3.hip's kernel under the same rule
      // (the round-3 choice), for A/B
      if (v == 0) attn_plan_v4(p, 16, big ? 8 : 4);
      else if (big) attn_plan_v3(p, 40, 2, 4, 3, 16, 8);
      else attn_plan_v3(p, 40, 2, 3, 3, 16, 4);
      return 0;
    }
    // head dim 80: only the shipped choice takes the 8-wave form
    attn_plan_v3(p, 80, 2, 2, 3, 16, v == 0 && big ? 8 : 4);
    return 0;
  }
  // attention.hip (fp32; bf16 at head dims 64 - the CLIP vision tower - and 160, or forced): 32 query rows per wave from 256
  // tokens up, key 2 = 1, 3 keep 16
  return attn_plan_v1(p, d, q.N >= 256 && v != 1 && v != 3 ? 2 : 1, false, false);
}

// launch_attention_fp8: bf16 qkv, fp8 (e4m3) operands
inline int attn_choose_fp8(const AttnKnobs& k, AttnPlan* p) {
  const AttnDesc& q = p->q;
  const int d = q.C / q.heads;
  p->pre_grid_y = q.heads; p->pre_grid_z = q.B;
  // head dim 40 on whole 128-key tiles: the 2x-rate block-scaled MFMAs
  if (k.mx_mode && d == 40 && q.N % kAttnMxTile == 0) {
    const int mv = q.N % 256 == 0 ? k.mx_variant : (k.mx_variant & 2);      // 8-wave workgroups own 256 queries
    p->form = ATTN_MX;
    p->D = 40; p->QF = 2; p->NST = 3; p->NWV = (mv & 1) ? 8 : 4; p->FEXP = (mv & 2) != 0;
    p->grid_x = (q.N / attn_v4_rows(p->NWV)) * q.heads * q.B;
    p->block = 64 * p->NWV;
    p->pre_grid_x = q.N / kAttnMxTile;
    p->scratch_bytes = (size_t)q.B * q.heads * (q.N / kAttnMxTile) * (kAttnMxKB + kAttnMxVB);
    return 0;
  }
  if (d != 40 && d != 80) return -2;
  p->form = ATTN_FP8;
  p->D = d; p->QF = 2; p->WPS = d == 40 ? 4 : 2; p->NST = 3;
  p->grid_x = attn_ceil(q.N, attn_v1_rows(p->QF)) * q.heads * q.B;
  p->pre_DP = d == 40 ? kAttnFp8DP40 : kAttnFp8DP80;
  const long per_bh = (long)q.N * (p->pre_DP / 16) * 2;           // 16-byte chunks of K and V per (image, head)
  p->pre_grid_x = per_bh > 256L * 256 ? 256 : (int)((per_bh + 255) / 256);
  p->scratch_bytes = (size_t)2 * q.B * q.heads * q.N * p->pre_DP;
  return 0;
}

// The whole decision for one launch of launch_attention / _causal / _fp8 / _cross: 0 and *out filled, or -2 = no such launch.
inline int attn_choose(const AttnDesc& q, const AttnKnobs& k, AttnPlan* out) {
  if (q.B < 1 || q.N < 1 || q.heads < 1 || q.C % q.heads != 0) return -2;
  AttnPlan p;
  p.q = q;
  int r = -2;
  switch (q.kind) {
    case ATTN_KIND_SELF: r = attn_choose_self(k, &p); break;
    case ATTN_KIND_CAUSAL:      // the CLIP text encoder: head dim 64 only, one 64-row query block against 64-key tiles
      if (q.C == 64 * q.heads) r = attn_plan_v1(&p, 64, 1, q.dtype == 2, true);
      break;
    case ATTN_KIND_FP8: r = attn_choose_fp8(k, &p); break;
    case ATTN_KIND_CROSS: {     // every product in fp32 on the VALU; dtype 2: the fp32 tensors of a bf16x3 handle
      const int d = q.C / q.heads;
      if (q.S < 1 || q.heads > 65535 || q.B > 65535 || q.dtype < 0 || q.dtype > 2 || (d != 40 && d != 80 && d != 160)) break;
      p.form = ATTN_CROSS;
      p.D = d;
      p.grid_x = attn_ceil(q.N, kAttnCrossRows); p.grid_y = q.heads; p.grid_z = q.B;
      r = 0;
      break;
    }
    default: break;
  }
  if (r == 0) *out = p;
  return r;
}

// The engine's rule for a transformer level of a handle with ldmseg_unet_set_attention_fp8(min_tokens): bf16, at least min_tokens
// tokens, and only where the fp8 path is the faster one - the mx form.  (The unscaled fp8 kernel that would serve head dim 80 /
// ragged lengths runs at the bf16 MFMA rate and measured SLOWER than the bf16 kernel - 222 vs 205 us at d = 80, N = 4096 - so a
// handle asked for fp8 from 4096 tokens up keeps that level in bf16.)  True: *out is the plan, out->scratch_bytes what to allocate.
inline bool attn_self_fp8_level(int B, int N, int C, int heads, int dtype, int min_tokens, const AttnKnobs& k, AttnPlan* out) {
  if (dtype != DT_BF16 || min_tokens <= 0 || N < min_tokens) return false;
  return attn_choose(AttnDesc{ATTN_KIND_FP8, B, N, 0, C, heads, DT_BF16}, k, out) == 0 && out->form == ATTN_MX;
}

// The dispatch-log name of launch `which` of a plan (the fp8 forms: 0 = the pre-pass, 1 = the attention kernel)
inline std::string attn_plan_name(const AttnPlan& p, int which = 0) {
  const char* t = p.q.dtype == DT_BF16 ? "bf16" : "f32";
  char b[64];
  switch (p.form) {
    case ATTN_V1:
      if (p.X3) std::snprintf(b, sizeof b, p.CAUSAL ? "attn_causal_x3<%d,%d>" : "attn_x3<%d,%d>", p.D, p.QF);
      else std::snprintf(b, sizeof b, p.CAUSAL ? "attn_causal<%s,%d,%d>" : "attn<%s,%d,%d>", t, p.D, p.QF);
      break;
    case ATTN_V3: std::snprintf(b, sizeof b, "attn3<%d,%d,%d,%d,0,%d,%d>", p.D, p.QF, p.WPS, p.NST, p.LAZY, p.NWV); break;
    case ATTN_V4: std::snprintf(b, sizeof b, "attn4<d40,%d,%d,%d>", p.NST, p.LAZY, p.NWV); break;
    case ATTN_FP8:
      if (which == 0) std::snprintf(b, sizeof b, "kv_to_fp8<%d,%d>", p.D, p.pre_DP);
      else std::snprintf(b, sizeof b, "attn_fp8<%d,%d,%d,%d>", p.D, p.QF, p.WPS, p.NST);
      break;
    case ATTN_MX:
      if (which == 0) std::snprintf(b, sizeof b, "kv_to_mx");
      else std::snprintf(b, sizeof b, "attn_mx<%d,%d,%d>", p.NST, p.NWV, p.FEXP ? 1 : 0);
      break;
    default: std::snprintf(b, sizeof b, "attention_cross_kernel<%s,%d>", t, p.D); break;
  }
  return b;
}
// "name grid=GXxGY block=T" (the pre-passes and the cross kernel, on 3-D grids: grid=GXxGYxGZ), the pre-pass of the fp8 forms
// first: "kv_to_mx grid=.. block=.. + attn_mx<3,8,1> grid=.. block=.."
inline std::string attn_plan_line(const AttnPlan& p) {
  char b[96];
  std::string s;
  if (p.form == ATTN_FP8 || p.form == ATTN_MX) {
    std::snprintf(b, sizeof b, " grid=%dx%dx%d block=%d + ", p.pre_grid_x, p.pre_grid_y, p.pre_grid_z, p.pre_block);
    s = attn_plan_name(p, 0) + b + attn_plan_name(p, 1);
  } else {
    s = attn_plan_name(p);
  }
  if (p.form == ATTN_CROSS) std::snprintf(b, sizeof b, " grid=%dx%dx%d block=%d", p.grid_x, p.grid_y, p.grid_z, p.block);
  else std::snprintf(b, sizeof b, " grid=%dx%d block=%d", p.grid_x, p.grid_y, p.block);
  return s + b;
}

}  // namespace ldmseg
