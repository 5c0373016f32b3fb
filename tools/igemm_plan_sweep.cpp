// The igemm chooser over a grid of launch descriptions, knob states and CU counts, on the host alone:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I latent-diffusion-segmentation_amd/csrc
//       tools/igemm_plan_sweep.cpp -o igemm_plan_sweep && ./igemm_plan_sweep
// Every accepted description must name a form the table has, with a grid inside the chip; prints how many launches each form took.
#include <cstdio>
#include <initializer_list>

#include "igemm_plan.h"

using namespace ldmseg;

int main() {
  const int Ms[] = {1, 27, 64, 500, 512, 1024, 2048, 3200, 8192, 18432, 32768, 65536, 131072};
  const int Ns[] = {32, 64, 96, 128, 160, 320, 640, 960, 1280, 2560, 3840, 10240};
  const int Cs[] = {32, 64, 320, 640, 1280, 2560, 5120};
  const int policies[] = {kDefaultPolicy, 0, 29, 63, 2, 16};
  const int cf_modes[] = {5, 0, 9, 13, 7 | (50 << 8)};
  const int cus_list[] = {256, 304, 64, 1};
  long per_form[kNarrowForm + 1] = {}, accepted = 0, rejected = 0;
  for (int dtype = 0; dtype < 2; ++dtype)
    for (int M : Ms) for (int N : Ns) for (int C0 : Cs) for (int var = 0; var < 8; ++var) for (int splits : {0, 1, 2, 4, 16, 40})
      for (int pol : policies) for (int force : {-1, 0, 2, 3, 9, 11, 12}) for (int cf : cf_modes) for (int cus : cus_list) {
        IgemmLaunchDesc q{M, N, C0, var == 1 ? C0 : 0, 0, 0, var == 2 ? 1 : 9, var == 3 ? 2 : 1, var == 4, 0, var == 5, var == 6, var == 7, 0, splits, 0, 1};
        if (var == 0) { q.taps = 9; q.C2 = C0; q.C3 = 64; }                       // extra tap
        if (var == 4 && M % 1024 == 0) { q.up = 0; q.up4 = 1; q.taps = 4; }      // phase convs
        if (var == 2 && dtype == DT_F32 && (C0 & 64)) q.x3 = 1 + (M & 1);        // split-bf16 without a LayerNorm
        if (var == 6) q.taps = 1;                                                // GEGLU
        if (var == 7) { q.taps = 1; q.x3 = dtype == DT_F32 ? 1 + (M & 1) : 0; }  // folded LayerNorm (+ split-bf16 in fp32)
        IgemmKnobs k;
        k.policy = pol; k.force_cfg = force; k.cf_mode = cf;
        k.cm_mode = pol & 1 ? -1 : 1; k.table_override = force == 3 ? (3 | (2 << 8)) : -1;
        if (q.splits == 0) q.splits = igemm_plan_splits_pure(q, dtype, k, cus);
        IgemmDispatch d;
        if (igemm_choose(q, dtype, k, cus, &d) != 0) { ++rejected; continue; }
        int f = -1;
        for (int i = 0; i <= kNarrowForm; ++i) {
          const IgemmForm& t = kIgemmForms[i];
          if (t.bm == d.bm && t.wm == d.wm && t.wn == d.wn && t.nst == d.nst && t.pipe == (d.pipe != 0) && t.ldr == d.ldr) f = i;
        }
        if (f < 0 || !igemm_form_exists(f, dtype, d.bn, d.lnf, d.cm, d.xt, d.up4) || d.grid < 1 || d.grid > 2 * cus || N % d.bn ||
            (d.cf && (d.grid > cus || d.splits < 2))) {
          std::printf("bad dispatch: M=%d N=%d C0=%d var=%d dtype=%d -> form %d bn %d grid %d\n", M, N, C0, var, dtype, f, d.bn, d.grid);
          return 1;
        }
        ++per_form[f]; ++accepted;
      }
  for (int i = 0; i <= kNarrowForm; ++i) std::printf("form %2d: %ld\n", i, per_form[i]);
  std::printf("%ld accepted, %ld rejected\n", accepted, rejected);
  return 0;
}
