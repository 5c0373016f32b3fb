// Which GroupNorm kernel a launch runs, on which grid and with which derived quantities: the forms norm.hip contains (GnForm,
// expanded by launch_gn_plan() there - the only place that names template arguments) and the rule that picks one (gn_choose,
// gn_finish_choose, gn_stats_choose).  Plain C++17: no HIP, no state - a function of the launch description, the knobs and the
// CU count, so it runs (and is tested, tests/test_gn_plan_cpu.py, tools/gn_plan_sweep.cpp) without a device.  DESIGN 3.3 has the
// rule as a table.
#pragma once
#include <cstdio>
#include <string>

#include "igemm_types.h"   // DType

namespace ldmseg {

// debug key 8 (GnKnobs::variant), a bit field
constexpr int kGnNoCoop = 1;         // no cooperative kernel (64x64 maps on the two-launch path); also switches gn_group off
constexpr int kGnCoopFrom256 = 2;    // cooperative kernel from 16x16 maps up
constexpr int kGnTwoPass = 4;        // two-pass gn_fused where gn_one would run
constexpr int kGnSplitFinish = 8;    // keep the split-K finish and the norm apart (finish_groupnorm_ok answers no)
constexpr int kGnRowstats1 = 16;     // one-row-per-wave rowstats (ln_choose, ln_plan.h)
constexpr int kGnNoGroup = 32;       // no gn_group
// variant: key 8; coop_mode (key 10): 1 = every cooperative workgroup computes its partners' records itself (tests of the cold
// path); poll_us (key 11): bound of the partner poll
struct GnKnobs { int variant = 0, coop_mode = 0, poll_us = 100; };

struct GnDesc { int B, HW, C0, C1, groups, nchunk, dtype; };

enum GnForm : int { GN_GROUP, GN_COOP, GN_ONE, GN_FUSED, GN_SMALL, GN_TWO_LAUNCH, GN_STATS, GN_FINISH };
// Template arguments (NV: gn_group's accesses per thread, 10 | 20; MAXV: vectors per thread of the register kernels, 2 | 6 | 12
// gn_one / finish_gn, 22 gn_fused, 21 gn_coop; GB: groups per workgroup), the launch (grid2: gn_apply's, after gn_partial on grid)
// and what the launcher writes into GNParams (div_*: the divisors behind fd_cpg / fd_vx / fd_aux; 1 = not read by the form).
struct GnPlan {
  int form = GN_TWO_LAUNCH, NV = 0, MAXV = 0, GB = 1;
  int grid_x = 1, grid_y = 1, grid2_x = 0, grid2_y = 0, block = 256;
  int splits = 1, per = 0, ty = 0, vx = 0, cpg = 0;
  double inv_n = 0.0;
  int div_cpg = 1, div_vx = 1, div_aux = 1;
};

constexpr int kGnMaxIter = 4;        // ceil(nvec / 256) the row kernels support (C * sizeof(T) / 16 <= 1024)
constexpr int kGnMaxSlabs = 2048;    // (image, group block) slabs a hand-off region of the cooperative kernel holds
constexpr int kGnCoopThreads = 512, kGnCoopMaxV = 21, kGnFusedMaxV = 22, kGnOneMaxV = 12;
constexpr int gn_pc(int dtype) { return dtype == DT_BF16 ? 8 : 4; }     // elements of a 16-byte vector
constexpr int gn_ceil(int a, int b) { return (a + b - 1) / b; }

// pixel chunks of the two-launch path: ~512-1024 workgroups in total, at least 8 pixels per chunk
inline int gn_nchunk_pure(int B, int HW) {
  int n = 768 / (B > 0 ? B : 1);
  if (n < 1) n = 1;
  if (n > 128) n = 128;
  while (n > 1 && HW / n < 8) n >>= 1;
  return n;
}

// what every form asks of a description (max_groups: 64, or 32 where statistics are combined by gn_reduce_stats)
inline bool gn_desc_ok(const GnDesc& q, int max_groups) {
  const int PC = gn_pc(q.dtype), C = q.C0 + q.C1;
  if (q.groups < 1 || C % q.groups != 0 || C % PC != 0 || q.C0 % PC != 0 || q.groups > max_groups) return false;
  // a 16-B vector may span at most two groups: cpg >= PC, or exactly two whole groups per vector
  // (128 channels in bf16: cpg 4, PC 8 - the image VAE's first level)
  if (C / q.groups < PC && 2 * (C / q.groups) != PC) return false;
  return C / PC <= 256 * kGnMaxIter;
}
inline GnPlan gn_plan_base(const GnDesc& q, int form) {
  GnPlan p;
  p.form = form;
  p.cpg = (q.C0 + q.C1) / q.groups;
  p.div_cpg = p.cpg;
  p.inv_n = 1.0 / ((double)q.HW * p.cpg);
  return p;
}

// 16-byte vectors per pixel of a block of GB groups; 0: the block is not whole vectors, does not divide the groups, or is wider
// than 64 vectors
inline int gn_block_vpp(int GB, int cpg, int groups, int PC) {
  if ((GB * cpg) % PC != 0 || groups % GB != 0) return 0;
  const int vpp = GB * cpg / PC;
  return vpp > 64 ? 0 : vpp;
}
// The block of the register-resident kernels (gn_one, gn_fused, finish_gn): GB groups per 256-thread workgroup, ppi pixels per
// trip, nv vectors per thread.  False: no such block, more than nv_cap vectors per thread, or fewer than 96 workgroups (too few
// to fill the chip).
struct GnBlock { int vpp, ppi, nv; };
inline bool gn_reg_block(int GB, int cpg, int groups, int PC, int B, int HW, int nv_cap, GnBlock* b) {
  b->vpp = gn_block_vpp(GB, cpg, groups, PC);
  if (!b->vpp) return false;
  b->ppi = 256 / b->vpp;
  b->nv = gn_ceil(HW, b->ppi);
  return b->nv <= nv_cap && (long)B * (groups / GB) >= 96;
}
inline void gn_plan_reg(GnPlan* p, int form, int GB, const GnBlock& b, int B, int groups) {
  p->form = form;
  p->GB = GB;
  p->MAXV = form == GN_FUSED ? kGnFusedMaxV : b.nv <= 2 ? 2 : b.nv <= 6 ? 6 : kGnOneMaxV;
  p->ty = b.ppi;
  p->div_aux = b.vpp;
  if (form == GN_FUSED) { p->grid_x = groups / GB; p->grid_y = B; }
  else p->grid_x = (groups / GB) * B;
}

// The rows of the two-launch path (gn_partial, gn_apply): vx threads per pixel row, ty pixel rows per trip, per pixels per chunk.
// False: it combines statistics with 8 lanes per group in a 256-thread workgroup (32 groups) and keeps at most 128 chunk partials
// per lane set (gn_reduce_stats: MAXP = 16 x 8 lanes).
inline bool gn_plan_rows(const GnDesc& q, GnPlan* p) {
  const int nvec = (q.C0 + q.C1) / gn_pc(q.dtype);
  p->vx = nvec < 256 ? nvec : 256;
  p->ty = 256 / p->vx;
  p->div_vx = p->vx;
  if (q.nchunk < 1 || q.nchunk > 128 || q.groups > 32) return false;
  p->per = gn_ceil(q.HW, q.nchunk);
  p->grid_x = q.nchunk;
  p->grid_y = q.B;
  return true;
}

// Statistics half of the two-launch path on its own (launch_groupnorm_stats): 0 and *out filled, or -2.
inline int gn_stats_choose(const GnDesc& q, GnPlan* out) {
  if (!gn_desc_ok(q, 32)) return -2;
  GnPlan p = gn_plan_base(q, GN_STATS);
  if (!gn_plan_rows(q, &p)) return -2;
  *out = p;
  return 0;
}

// Split-K finish + GroupNorm(32) in one launch (finish_gn): 0 and *out filled, or -4 = conv and norm run apart (no instantiation
// for the shape, or kGnSplitFinish).  The block rule of gn_one with its cap; kGnTwoPass is not consulted (there is no two-pass
// finish kernel).
inline int gn_finish_choose(int B, int HW, int C, int dtype, const GnKnobs& k, GnPlan* out) {
  if ((k.variant & kGnSplitFinish) || C % 32 != 0) return -4;
  const GnDesc q{B, HW, C, 0, 32, 0, dtype};
  GnPlan p = gn_plan_base(q, GN_FINISH);
  for (int GB = 1; GB <= 2; ++GB) {
    GnBlock b;
    if (!gn_reg_block(GB, p.cpg, 32, gn_pc(dtype), B, HW, kGnOneMaxV, &b)) continue;
    gn_plan_reg(&p, GN_FINISH, GB, b, B, 32);
    *out = p;
    return 0;
  }
  return -4;
}

// The whole decision for one launch_groupnorm: 0 and *out filled, or -2 = no such launch.  region_ok: a hand-off region exists
// for the stream (without one no cooperative kernel runs at any GB, and the rest of the rule applies).
inline int gn_choose(const GnDesc& q, const GnKnobs& k, int cus, bool region_ok, GnPlan* out) {
  if (!gn_desc_ok(q, 64)) return -2;
  const int PC = gn_pc(q.dtype), B = q.B, HW = q.HW, groups = q.groups;
  GnPlan p = gn_plan_base(q, GN_TWO_LAUNCH);
  const int cpg = p.cpg;
  // gn_group - one workgroup per (image, group) with the slice in registers, where that slice is small enough for 8-byte pieces to
  // win (<= 40 dwords per thread and channels per group a multiple of 4; bf16).  Measured at B = 8, kbench gn: 32x32 x 640
  // 12.0 -> 7.5 us (11 norms of a forward), 32x32 x (640+640) 15.5 -> 12.0, 16x16 x 640 6.1 -> 4.4, 16x16 x 1280 6.4 -> 5.2,
  // 16x16 x (1280+1280) 9.3 -> 6.9, 16x16 x (1280+640) 10.4 -> 7.5; 8x8 maps level with gn_one and left there; whole forward
  // -0.07 ms.  The 4-byte prototype lost from 40 dwords per thread up (64x64 x 320: 20.5 against 16.6 us, TA-bound).
  if (q.dtype == DT_BF16) {
    const long acc8 = (long)HW * (cpg / 4);                       // 8-byte accesses per (image, group) slice
    if (!(k.variant & (kGnNoCoop | kGnNoGroup)) && HW >= 256 && cpg % 4 == 0 && cpg <= 128 && q.C0 % 4 == 0 && q.C1 % 4 == 0 &&
        acc8 <= 512L * 20 && (long)B * groups >= 128) {
      p.form = GN_GROUP;
      p.NV = acc8 <= 512 * 10 ? 10 : 20;
      p.grid_x = B * groups;
      p.block = 512;
      *out = p;
      return 0;
    }
  }
  // gn_coop - the cooperative one-pass kernel first from 32x32 maps up: the maps the register-resident kernels cannot hold (64x64
  // and up), and (measured at B = 8) 32x32 x 640 13.9 -> 11.7 us, 32x32 x 1920 29.1 -> 18.8 us, 64x64 x 320 22.9 -> 16.3 us against
  // the forms below.  (One attempt: an attempt after the register kernels would see the same description, CU count and region and
  // fail as this one did.)
  if (region_ok && !(k.variant & kGnNoCoop) && HW >= ((k.variant & kGnCoopFrom256) ? 256 : 1024)) {
    for (int GB = 1; GB <= 4; GB *= 2) {
      const int vpp = cpg < PC || cpg % 2 != 0 ? 0 : gn_block_vpp(GB, cpg, groups, PC);
      if (!vpp) continue;
      const int ppi = kGnCoopThreads / vpp;
      const int slabs = B * (groups / GB);
      if (slabs > kGnMaxSlabs) continue;
      // splits: enough workgroups for every CU, as few as the registers allow
      int S = 1;
      while (S < 8 && gn_ceil(gn_ceil(HW, S), ppi) > kGnCoopMaxV) S *= 2;
      while (S < 8 && slabs * S * 2 <= cus && HW / (2 * S) >= ppi) S *= 2;
      if (gn_ceil(gn_ceil(HW, S), ppi) > kGnCoopMaxV) continue;
      if (slabs * S > cus) continue;                              // every workgroup must be resident: one per CU (8 waves at ~200 registers)
      p.form = GN_COOP;
      p.GB = GB;
      p.MAXV = kGnCoopMaxV;
      p.grid_x = slabs * S;
      p.block = kGnCoopThreads;
      p.splits = S;
      p.per = gn_ceil(HW, S);
      p.ty = ppi;
      p.div_aux = vpp;
      p.div_vx = S;
      p.div_cpg = groups / GB;                                    // (the kernel divides a slab by the group blocks of an image)
      *out = p;
      return 0;
    }
  }
  // gn_one / gn_fused - single-launch register-resident kernels: GB = 1 or 2 groups per workgroup forming whole 16-byte vectors
  for (int GB = 1; GB <= 2; ++GB) {
    GnBlock b;
    if (!gn_reg_block(GB, cpg, groups, PC, B, HW, kGnFusedMaxV, &b)) continue;
    // gn_one: one reduction, one barrier; measured at B = 8: 8x8 x 1280 6.2 -> 4.1 us, 16x16 x 1280 7.9 -> 6.9 us; with more than
    // 12 vectors per thread the two-pass gn_fused is the faster one (16x16 x 1920: 10.2 against 11.4 us)
    const bool one = !(k.variant & kGnTwoPass) && b.nv <= kGnOneMaxV;
    if (!one && HW <= 64 && b.vpp < 10) continue;                 // 8x8 maps with short runs: gn_small measured faster (8.0 vs 9.7 us)
    gn_plan_reg(&p, one ? GN_ONE : GN_FUSED, GB, b, B, groups);
    *out = p;
    return 0;
  }
  // gn_small - measured: wins for the 8x8 maps (16 -> 9 us), loses from 16x16 up (its 4-byte strided loads)
  const int EPU = q.dtype == DT_BF16 ? 2 : 1;                     // elements of a 4-byte unit
  if (cpg % EPU == 0 && q.C0 % EPU == 0 && (long)HW * (cpg / EPU) <= 256 * 12 && (long)B * groups >= 128) {
    p.form = GN_SMALL;
    p.MAXV = 12;
    p.grid_x = groups;
    p.grid_y = B;
    p.div_aux = cpg / EPU;
    *out = p;
    return 0;
  }
  // gn_partial + gn_apply
  if (!gn_plan_rows(q, &p)) return -2;
  // gn_apply: 16 pixels per thread row (4 unrolled trips) on the big maps, down to 4 when that would leave fewer than ~512
  // workgroups on the chip (every workgroup re-reduces the image's partials first, so fewer and fatter is better)
  int blocks = gn_ceil(HW, 16 * p.ty);
  const int want = 512 / B > 1 ? 512 / B : 1, few = gn_ceil(HW, 4 * p.ty);
  if (blocks < want) blocks = want < few ? want : few;
  const int cap = 1024 / B > 1 ? 1024 / B : 1;
  if (blocks > cap) blocks = cap;
  p.grid2_x = blocks < 1 ? 1 : blocks;
  p.grid2_y = B;
  *out = p;
  return 0;
}

// The dispatch-log name of launch `which` (0; 1 = gn_apply of the two-launch form) of a plan
inline std::string gn_plan_name(const GnPlan& p, int dtype, int which = 0) {
  const char* t = dtype == DT_BF16 ? "bf16" : "f32";
  char b[64];
  switch (p.form) {
    case GN_GROUP: std::snprintf(b, sizeof b, "gn_group<bf16,%d,2>", p.NV); break;
    case GN_COOP: std::snprintf(b, sizeof b, "gn_coop<%s,%d,%d,GB=%d>", t, p.MAXV, p.block, p.GB); break;
    case GN_ONE: std::snprintf(b, sizeof b, "gn_one<%s,%d,GB=%d>", t, p.MAXV, p.GB); break;
    case GN_FUSED: std::snprintf(b, sizeof b, "gn_fused<%s,%d,GB=%d>", t, p.MAXV, p.GB); break;
    case GN_SMALL: std::snprintf(b, sizeof b, "gn_small<%s,%d>", t, p.MAXV); break;
    case GN_FINISH: std::snprintf(b, sizeof b, "finish_gn<%s,%d,GB=%d>", t, p.MAXV, p.GB); break;
    default: std::snprintf(b, sizeof b, which ? "gn_apply<%s>" : "gn_partial<%s>", t); break;
  }
  return b;
}
// "name[ + name] splits=S grid=GXxGY[+GXxGY] block=T"
inline std::string gn_plan_line(const GnPlan& p, int dtype) {
  std::string s = gn_plan_name(p, dtype);
  char b[96];
  if (p.form == GN_TWO_LAUNCH) {
    s += " + " + gn_plan_name(p, dtype, 1);
    std::snprintf(b, sizeof b, " splits=%d grid=%dx%d+%dx%d block=%d", p.splits, p.grid_x, p.grid_y, p.grid2_x, p.grid2_y, p.block);
  } else {
    std::snprintf(b, sizeof b, " splits=%d grid=%dx%d block=%d", p.splits, p.grid_x, p.grid_y, p.block);
  }
  return s + b;
}

}  // namespace ldmseg
