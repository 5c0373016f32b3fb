// Which kernel a LayerNorm (launch_layernorm) or a row-statistics pass (launch_rowstats) runs and on which grid: the forms norm.hip
// contains (LnForm, expanded by launch_ln_plan() there - the only place that names their template arguments) and the rule that
// picks one (ln_choose).  Plain C++17: no HIP, no state - a function of the launch description and the knobs, so it runs (and is
// tested, tests/test_ln_plan_cpu.py) without a device.
#pragma once
#include <cstdio>
#include <string>

#include "gn_plan.h"       // GnKnobs, kGnRowstats1, gn_pc

namespace ldmseg {

// M rows of C channels; stats: 1 = only (mean, rstd) per row are written (launch_rowstats), 0 = the rows are normalised
struct LnDesc { int M, C, dtype, stats; };

// LN_ROWS: layernorm_kernel<T, VPL, RPW[, stats]> - a wave per row, VPL 16-byte vectors per lane, RPW rows in flight per wave.
// LN_SHARED: rowstats_kernel<T, LPR, RPW> - LPR lanes share a row (5 vectors per lane), 64 / LPR rows per butterfly.
enum LnForm : int { LN_ROWS, LN_SHARED };
struct LnPlan {
  int form = LN_ROWS, stats = 0;
  int VPL = 0, LPR = 0, RPW = 0;   // VPL: LN_ROWS; LPR: LN_SHARED
  int grid_x = 1, block = 256;     // four waves per workgroup
};

constexpr int kLnSharedVPL = 5;    // vectors per lane of rowstats_kernel: 8 lanes x 5 = the 40 vectors of a 320-channel bf16 row
constexpr int kLnRowsGridCap = 2048, kLnSharedGridCap = 4096;   // workgroups; the kernels grid-stride over row batches beyond (values as recorded)

// workgroups for M rows at `rows` rows per four-wave workgroup and trip, capped
inline int ln_grid(int M, int rows, int cap) {
  const int blocks = (M + rows - 1) / rows;
  return blocks > cap ? cap : blocks < 1 ? 1 : blocks;
}

// The whole decision for one launch: 0 and *out filled, or -2 = no such launch (a row that is not whole 16-byte vectors, or one
// wider than 5 vectors per lane of a wave).
inline int ln_choose(const LnDesc& q, const GnKnobs& k, LnPlan* out) {
  const int PC = gn_pc(q.dtype);
  if (q.C % PC != 0) return -2;
  const int nvec = q.C / PC;
  LnPlan p;
  p.stats = q.stats ? 1 : 0;
  // statistics: LPR = 8 / 16 / 32 / 64 lanes share a row of up to 5 * LPR vectors, two batches of rows in flight per wave
  // (no lane idles on the 40-vector rows; 187 -> 172 us per forward).  kGnRowstats1 keeps the one-row-per-wave form.
  if (p.stats && !(k.variant & kGnRowstats1) && nvec <= 64 * kLnSharedVPL) {
    p.form = LN_SHARED;
    p.LPR = nvec <= 8 * kLnSharedVPL ? 8 : nvec <= 16 * kLnSharedVPL ? 16 : nvec <= 32 * kLnSharedVPL ? 32 : 64;
    p.RPW = 2;
    p.grid_x = ln_grid(q.M, 4 * (64 / p.LPR) * p.RPW, kLnSharedGridCap);
    *out = p;
    return 0;
  }
  // a wave per row: vpl = vectors per lane the row needs; the instantiations are VPL 1, 2, 3 and 5 (vpl 4 runs the VPL 5 code),
  // with fewer rows in flight the more registers a row takes (4, 4, 2 rows; as recorded)
  const int vpl = (nvec + 63) / 64;
  if (vpl < 1 || vpl > 5) return -2;
  p.VPL = vpl <= 3 ? vpl : 5;
  // VPL 5: one row in flight where the rows are normalised, two in the statistics form, which keeps no gamma / beta in registers
  // (as recorded)
  p.RPW = vpl <= 2 ? 4 : vpl == 3 ? 2 : p.stats ? 2 : 1;
  p.grid_x = ln_grid(q.M, 4 * p.RPW, kLnRowsGridCap);
  *out = p;
  return 0;
}

// The dispatch-log name of a plan's launch
inline std::string ln_plan_name(const LnPlan& p, int dtype) {
  const char* t = dtype == DT_BF16 ? "bf16" : "f32";
  char b[64];
  if (p.form == LN_SHARED) std::snprintf(b, sizeof b, "rowstats<%s,%d,%d>", t, p.LPR, p.RPW);
  else std::snprintf(b, sizeof b, p.stats ? "layernorm<%s,%d,%d,stats>" : "layernorm<%s,%d,%d>", t, p.VPL, p.RPW);
  return b;
}
// "name grid=GX block=T"
inline std::string ln_plan_line(const LnPlan& p, int dtype) {
  char b[48];
  std::snprintf(b, sizeof b, " grid=%d block=%d", p.grid_x, p.block);
  return ln_plan_name(p, dtype) + b;
}

}  // namespace ldmseg
