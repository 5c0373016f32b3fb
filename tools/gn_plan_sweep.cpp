// The GroupNorm chooser over a grid of launch descriptions, knob states, both region answers and CU counts, on the host alone:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I latent-diffusion-segmentation_amd/csrc
//       tools/gn_plan_sweep.cpp -o gn_plan_sweep && ./gn_plan_sweep
// Every plan must name an instantiation norm.hip has, with vectors per thread inside the form's cap, at most 64 vectors per pixel,
// a grid of at least one workgroup and - the cooperative form - no more workgroups than CUs; prints how many launches each form took.
#include <cstdio>
#include <initializer_list>

#include "gn_plan.h"

using namespace ldmseg;

static const char* bad_plan(const GnDesc& q, const GnPlan& p, int cus, bool region_ok) {
  const int PC = gn_pc(q.dtype), cpg = (q.C0 + q.C1) / q.groups;
  if (p.grid_x < 1 || p.grid_y < 1 || p.cpg != cpg || p.div_cpg < 1 || p.div_vx < 1 || p.div_aux < 1) return "grid / divisors";
  const int vpp = p.GB * cpg / PC;
  switch (p.form) {
    case GN_GROUP:
      if (q.dtype != DT_BF16 || (p.NV != 10 && p.NV != 20) || p.block != 512 || (long)q.HW * (cpg / 4) > 512L * p.NV) return "gn_group";
      break;
    case GN_COOP:
      if (!region_ok || p.MAXV != 21 || p.block != 512 || (p.GB != 1 && p.GB != 2 && p.GB != 4) || vpp < 1 || vpp > 64 || p.div_aux != vpp ||
          p.grid_x > cus || p.splits < 1 || p.splits > 8 || (p.splits & (p.splits - 1)) || p.ty != 512 / vpp ||
          gn_ceil(p.per, p.ty) > p.MAXV || (long)p.per * p.splits < q.HW || p.grid_x != q.B * (q.groups / p.GB) * p.splits ||
          q.B * (q.groups / p.GB) > kGnMaxSlabs)
        return "gn_coop";
      break;
    case GN_ONE: case GN_FUSED: case GN_FINISH: {
      const bool one = p.form != GN_FUSED;
      if ((one ? p.MAXV != 2 && p.MAXV != 6 && p.MAXV != 12 : p.MAXV != 22) || (p.GB != 1 && p.GB != 2) || vpp < 1 || vpp > 64 ||
          p.div_aux != vpp || p.ty != 256 / vpp || gn_ceil(q.HW, p.ty) > p.MAXV || p.block != 256 ||
          (long)p.grid_x * p.grid_y != (long)q.B * (q.groups / p.GB))
        return "register kernel";
      break;
    }
    case GN_SMALL:
      if (p.MAXV != 12 || (long)q.HW * p.div_aux > 256 * 12 || p.grid_x != q.groups || p.grid_y != q.B) return "gn_small";
      break;
    case GN_TWO_LAUNCH: case GN_STATS:
      if (p.vx < 1 || p.vx > 256 || p.ty != 256 / p.vx || p.div_vx != p.vx || (long)p.per * q.nchunk < q.HW || p.grid_x != q.nchunk ||
          p.grid_y != q.B || q.groups > 32 || (p.form == GN_TWO_LAUNCH && (p.grid2_x < 1 || p.grid2_y != q.B)))
        return "two launches";
      break;
    default: return "form";
  }
  return gn_plan_line(p, q.dtype).empty() ? "name" : nullptr;
}

int main() {
  const int Bs[] = {1, 2, 3, 4, 5, 8, 16, 32, 100}, Cs[] = {32, 64, 96, 128, 256, 320, 512, 640, 960, 1280, 1920, 2560, 4096, 8192};
  const int HWs[] = {1, 4, 16, 63, 64, 100, 255, 256, 400, 1023, 1024, 1156, 2047, 2048, 3969, 4096, 16384, 65536};
  long per_form[GN_FINISH + 1] = {}, rejected = 0;
  for (int dtype = 0; dtype < 2; ++dtype)
    for (int B : Bs) for (int C : Cs) for (int cat = 0; cat < 3; ++cat) for (int HW : HWs) for (int groups : {32, 16, 64, 1, 0, 128})
      for (int variant = 0; variant < 64; ++variant) {
        const int C0 = cat == 0 ? C : cat == 1 ? C / 2 : C - 4;
        const GnDesc q{B, HW, C0, C - C0, groups, gn_nchunk_pure(B, HW), dtype};
        const GnKnobs k{variant, variant & 1, 100};
        GnPlan p;
        for (int cus = 64; cus <= 304; cus += 48)
          for (int region_ok = 0; region_ok < 2; ++region_ok) {
            if (gn_choose(q, k, cus, region_ok != 0, &p) != 0) { ++rejected; continue; }
            if (const char* why = bad_plan(q, p, cus, region_ok != 0)) {
              std::printf("bad plan (%s): B=%d HW=%d C0=%d C1=%d groups=%d dtype=%d variant=%d cus=%d -> %s\n", why, B, HW, q.C0, q.C1, groups,
                          dtype, variant, cus, gn_plan_line(p, dtype).c_str());
              return 1;
            }
            ++per_form[p.form];
          }
        if (gn_stats_choose(q, &p) == 0) {
          if (bad_plan(q, p, 256, false)) { std::printf("bad statistics plan: B=%d HW=%d C=%d\n", B, HW, C); return 1; }
          ++per_form[GN_STATS];
        }
        if (cat == 0 && groups == 32 && gn_finish_choose(B, HW, C, dtype, k, &p) == 0) {
          if (bad_plan(q, p, 256, false) || (variant & kGnSplitFinish)) { std::printf("bad finish plan: B=%d HW=%d C=%d\n", B, HW, C); return 1; }
          ++per_form[GN_FINISH];
        }
      }
  const char* names[] = {"gn_group", "gn_coop", "gn_one", "gn_fused", "gn_small", "gn_partial + gn_apply", "gn_partial", "finish_gn"};
  for (int f = 0; f <= GN_FINISH; ++f) {
    std::printf("%-22s %ld\n", names[f], per_form[f]);
    if (!per_form[f]) { std::printf("form never chosen\n"); return 1; }
  }
  std::printf("%ld rejected\n", rejected);
  return 0;
}
