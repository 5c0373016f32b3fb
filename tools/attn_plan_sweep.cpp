// The attention chooser over a grid of launch descriptions and knob states, on the host alone:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I latent-diffusion-segmentation_amd/csrc
//       tools/attn_plan_sweep.cpp -o attn_plan_sweep && ./attn_plan_sweep
// Every plan must name an instantiation its source file has, on a grid whose workgroups cover every query row of every (image,
// head) exactly (the mx kernel has no ragged form: its rows per workgroup must divide N), with a scratch that holds what the
// pre-pass writes; prints how many launches each form took and - build it with -O2 and without the sanitizers for this - the host
// time of one attn_choose (one per attention launch, 16 per forward).
#include <chrono>
#include <cstdio>
#include <initializer_list>

#include "attn_plan.h"

using namespace ldmseg;

static const char* bad_plan(const AttnDesc& q, const AttnPlan& p) {
  const long bh = (long)q.B * q.heads;
  const int d = q.C / q.heads;
  if (p.D != d || p.grid_x < 1 || p.block < 64 || p.block > 512) return "head dim / launch";
  int rows = 0;
  switch (p.form) {
    case ATTN_V1:
      if ((d != 40 && d != 64 && d != 80 && d != 160) || (p.QF != 1 && p.QF != 2) || (d == 160 && p.QF != 1) || p.block != 256 ||
          (p.CAUSAL && (d != 64 || p.QF != 1)) || p.X3 != (q.dtype == 2))
        return "attention.hip";
      rows = attn_v1_rows(p.QF);
      break;
    case ATTN_V3:
      if (q.dtype != DT_BF16 || (d != 40 && d != 80) || (p.NWV != 4 && p.NWV != 8) || p.block != 64 * p.NWV || p.NST < 2 || p.NST > 3)
        return "attention3.hip";
      rows = attn_v3_rows(p.QF, p.NWV);
      break;
    case ATTN_V4:
      if (q.dtype != DT_BF16 || d != 40 || (p.NWV != 4 && p.NWV != 8) || p.block != 64 * p.NWV || p.NST != 2 || (p.LAZY != 1 && p.LAZY != 16))
        return "attention4.hip";
      rows = attn_v4_rows(p.NWV);
      break;
    case ATTN_FP8:
      if ((d != 40 && d != 80) || p.block != 256 || p.pre_DP < d + 2 || p.pre_DP % 16 || p.pre_grid_x < 1 || p.pre_grid_x > 256 ||
          p.pre_grid_y != q.heads || p.pre_grid_z != q.B || p.scratch_bytes != (size_t)2 * bh * q.N * p.pre_DP)
        return "attention_fp8.hip";
      rows = attn_v1_rows(p.QF);
      break;
    case ATTN_MX:
      if (d != 40 || (p.NWV != 4 && p.NWV != 8) || p.block != 64 * p.NWV || q.N % kAttnMxTile || q.N % attn_v4_rows(p.NWV) ||
          p.pre_grid_x != q.N / kAttnMxTile || p.pre_grid_y != q.heads || p.pre_grid_z != q.B ||
          p.scratch_bytes != (size_t)bh * (q.N / kAttnMxTile) * (kAttnMxKB + kAttnMxVB))
        return "attention_mx.hip";
      rows = attn_v4_rows(p.NWV);
      break;
    case ATTN_CROSS:
      if ((d != 40 && d != 80 && d != 160) || p.block != 256 || p.grid_y != q.heads || p.grid_z != q.B || p.grid_x != attn_ceil(q.N, kAttnCrossRows))
        return "attention_cross.hip";
      return attn_plan_line(p).empty() ? "name" : nullptr;
    default: return "form";
  }
  if ((long)p.grid_x != attn_ceil(q.N, rows) * bh || p.grid_y != 1 || p.grid_z != 1) return "grid";
  return attn_plan_line(p).empty() ? "name" : nullptr;
}

int main() {
  const int Ns[] = {1, 33, 64, 127, 128, 200, 255, 256, 257, 384, 768, 769, 1000, 1024, 4096, 5184, 16384}, Bs[] = {1, 2, 3, 4, 8, 16, 32};
  const int Ds[] = {40, 48, 64, 80, 160, 0, 41};
  long per_form[ATTN_CROSS + 1] = {}, rejected = 0, calls = 0;
  const auto t0 = std::chrono::steady_clock::now();
  for (int kind = 0; kind < 5; ++kind)
    for (int dtype = 0; dtype < 4; ++dtype)
      for (int B : Bs) for (int N : Ns) for (int d : Ds) for (int heads : {8, 1, 12, 16, 0, -1})
        for (int variant = -1; variant < 17; ++variant) for (int mx = 0; mx < 8; ++mx) {
          const AttnDesc q{kind, B, N, kind == ATTN_KIND_CROSS ? 77 : 0, d ? d * heads : 100, heads, dtype};
          const AttnKnobs k{variant, mx & 1, mx >> 1};
          AttnPlan p;
          ++calls;
          if (attn_choose(q, k, &p) != 0) { ++rejected; continue; }
          if (const char* why = bad_plan(q, p)) {
            std::printf("bad plan (%s): kind=%d B=%d N=%d C=%d heads=%d dtype=%d key2=%d mx=%d -> %s\n", why, kind, B, N, q.C, heads, dtype,
                        variant, mx, attn_plan_line(p).c_str());
            return 1;
          }
          ++per_form[p.form];
          AttnPlan lv;
          if (attn_self_fp8_level(B, N, q.C, heads, dtype, 4096, k, &lv) && (lv.form != ATTN_MX || N < 4096 || dtype != DT_BF16 || !lv.scratch_bytes)) {
            std::printf("bad fp8 level: B=%d N=%d C=%d\n", B, N, q.C);
            return 1;
          }
        }
  const double ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
  const char* names[] = {"attention.hip", "attention3.hip", "attention4.hip", "attention_fp8.hip", "attention_mx.hip", "attention_cross.hip"};
  for (int f = 0; f <= ATTN_CROSS; ++f) {
    std::printf("%-20s %ld\n", names[f], per_form[f]);
    if (!per_form[f]) { std::printf("form never chosen\n"); return 1; }
  }
  std::printf("%ld rejected\n%ld descriptions, %.1f ns each (attn_choose, the plan check and attn_self_fp8_level)\n", rejected, calls, ns / calls);
  // the chooser alone, on the shipped knobs and the four self-attention levels of a forward
  const AttnDesc levels[] = {{ATTN_KIND_SELF, 8, 4096, 0, 320, 8, 1}, {ATTN_KIND_SELF, 8, 1024, 0, 640, 8, 1}, {ATTN_KIND_SELF, 8, 256, 0, 1280, 8, 1},
                             {ATTN_KIND_SELF, 8, 64, 0, 1280, 8, 1}};
  const AttnKnobs k;
  long sum = 0;
  const int reps = 2000000;
  const auto t1 = std::chrono::steady_clock::now();
  for (int i = 0; i < reps; ++i) {
    AttnPlan p;
    AttnDesc q = levels[i & 3];
    q.B += i & 1;                       // (keeps the call from being hoisted)
    if (attn_choose(q, k, &p) == 0) sum += p.grid_x;
  }
  const double ns1 = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t1).count();
  std::printf("attn_choose alone: %.1f ns per call (%d calls, checksum %ld)\n", ns1 / reps, reps, sum);
  return 0;
}
