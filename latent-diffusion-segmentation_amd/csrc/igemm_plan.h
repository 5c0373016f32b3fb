// Which igemm_kernel instantiation a launch runs, on how many K slices and workgroups: the tile forms the library contains
// (LDMSEG_IGEMM_FORMS, expanded again by launch_tile() in igemm.hip - the only place that names template arguments) and the rule
// that picks one (igemm_choose).  Plain C++17: no HIP, no state - a function of the launch description, the knobs and the CU
// count, so it runs (and is tested, tests/test_igemm_plan_cpu.py) without a device.
#pragma once
#include <cstddef>

#include "igemm_types.h"

namespace ldmseg {

// policy: bit0 8-wave 256-row tiles with a 3-stage ring (-0.15 ms per forward, on); bit1 4-stage ring, one workgroup per CU, for
// mid-size grids (+0.5 ms, off); bit2 lone 64-row 4-stage tiles; bit3 pipelined K loop on the 256-row tiles; bit4 8-wave 128-row
// tiles (+ loader waves on long K); bit5 loader waves on the 256-row tiles (long K / GEGLU).  force_cfg (debug key 5,
// tools/tune_igemm.py): every launch runs this entry of LDMSEG_IGEMM_FORMS.  Keys 23, 9, 24, 19, 21 for the rest: kernels.h.
constexpr int kDefaultPolicy = 61;
struct IgemmKnobs { int policy = kDefaultPolicy, force_cfg = -1, cf_mode = 5, cm_mode = -1, table_override = -1, xt_mode = 1, up4_mode = 1; };
constexpr size_t kIgemmCfBytes = 64 << 10;   // counter region of the in-launch finish

// The tile forms, one per line: X(BM, WAVES_M, WAVES_N, NST, PIPE, LDR, WIDE, LN, XT, UP4, CM, CF).  A form exists in bf16 and
// fp32, on 160- and 128-column tiles (WIDE) or 64- and 32-column ones (!WIDE); LN: also with a folded LayerNorm; XT / UP4 / CM:
// also with the extra centre tap / as four phase convs / in channel-major K order (each bf16, 160 columns, no LayerNorm);
// CF: its bf16 160-column instantiations without LayerNorm and CM have a twin that finishes the K slices inside the launch.
// The first twelve lines are the entries the launch table (igemm_tuned.inc) and debug keys 5 / 24 index, in this order.
//   10 / 11: the M = 512 .. 2048 1x1 launches.  (Entry 9 re-reads the W fragments in each of its four wave rows, 98 KB per K tile
//   against 56 KB here, and its compute waves issue the LDS-DMA themselves: 17.0 -> 13.6 us at M = 2048, N = K = 1280)
#define LDMSEG_IGEMM_FORMS(X)                                                                                          \
  X(256, 4, 2, 3, true, 4, true, true, true, true, true, true)         /*  0  256 rows, 8 compute + 4 loader waves */ \
  X(256, 4, 2, 3, true, 0, true, true, false, false, false, false)     /*  1  256 rows, 8 waves, pipelined K loop */   \
  X(256, 4, 2, 3, false, 0, true, false, false, false, false, false)   /*  2  256 rows, 8 waves, plain K loop */       \
  X(128, 2, 2, 4, true, 4, true, false, true, false, false, true)      /*  3  128 rows, 4 compute + 4 loader waves, 4-stage ring */ \
  X(128, 4, 2, 3, true, 0, true, true, true, false, false, true)       /*  4  128 rows, 8 waves, pipelined K loop */   \
  X(128, 2, 2, 4, false, 0, true, false, false, false, false, false)   /*  5  128 rows, 4 waves, 4-stage ring (one workgroup per CU) */ \
  X(64, 2, 2, 4, false, 0, true, true, false, false, false, false)     /*  6  64 rows, 4 waves, 4-stage ring */        \
  X(64, 2, 2, 2, false, 0, true, true, false, false, false, false)     /*  7  64 rows, 4 waves, two workgroups per CU */ \
  X(128, 2, 2, 2, false, 0, true, true, false, false, false, false)    /*  8  128 rows, 4 waves, two workgroups per CU */ \
  X(64, 4, 2, 4, false, 0, true, false, false, false, false, false)    /*  9  64 rows, 8 waves (16 x 80 wave tiles), 4-stage ring */ \
  X(64, 2, 2, 4, true, 4, true, false, false, false, false, true)      /* 10  64 rows, 4 compute (32 x 80 wave tiles) + 4 loader waves, 4-stage ring */ \
  X(64, 2, 2, 3, true, 4, true, false, false, false, false, false)     /* 11  the same on a 3-stage ring */            \
  X(128, 4, 1, 2, false, 0, false, false, false, false, false, false)  /* 12  128 rows x 64 / 32 columns: the narrow outputs */
struct IgemmForm { int bm, wm, wn, nst; bool pipe; int ldr; bool wide, ln, xt, up4, cm, cf; };
#define LDMSEG_IGEMM_FORM_ROW(BM, WM, WN, NST, PIPE, LDR, WIDE, LN, XT, UP4, CM, CF) {BM, WM, WN, NST, PIPE, LDR, WIDE, LN, XT, UP4, CM, CF},
constexpr IgemmForm kIgemmForms[] = {LDMSEG_IGEMM_FORMS(LDMSEG_IGEMM_FORM_ROW)};
#undef LDMSEG_IGEMM_FORM_ROW
// the entries a table / a debug key may name: the WIDE lines, which come first; the narrow form is the line after them
constexpr int igemm_wide_forms() { int n = 0; for (const IgemmForm& f : kIgemmForms) n += f.wide ? 1 : 0; return n; }
constexpr int kNumCfg = igemm_wide_forms();
constexpr int kNarrowForm = kNumCfg;
static_assert(sizeof(kIgemmForms) / sizeof(kIgemmForms[0]) == kNarrowForm + 1 && !kIgemmForms[kNarrowForm].wide, "form table");
// whether form f has an instantiation for (dtype, N tile, folded LayerNorm, CM / XT / UP4)
constexpr bool igemm_form_exists(int f, int dtype, int bn, bool lnf, bool cm, bool xt, bool up4) {
  const IgemmForm& t = kIgemmForms[f];
  if (cm || xt || up4) return dtype == DT_BF16 && bn == 160 && !lnf && (cm ? t.cm : xt ? t.xt : t.up4);
  return (t.wide ? bn == 160 || bn == 128 : bn == 64 || bn == 32) && (!lnf || t.ln);
}
// Launch table measured on the MI355X (tools/tune_igemm.py): launch shape -> entry of LDMSEG_IGEMM_FORMS + number of K slices.
// Shapes that are not listed (other batch sizes, other models) use the rules below; so does every launch while a non-default
// tile policy is set (tests, ablations).
struct IgemmTuned { int dtype, M, N, K, taps, stride, up, epi, lnf, cfg, splits; };
constexpr IgemmTuned kIgemmTuned[] = {
#include "igemm_tuned.inc"
    {-1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}};
// the table's answer for a launch: cfg < 0 = none.  An extra tap is ignored (K is the 3x3 part's), so a conv2 + conv_shortcut
// launch inherits the entry of the conv it extends.
struct IgemmTableHit { int cfg, splits; };
inline IgemmTableHit igemm_table(const IgemmLaunchDesc& q, int dtype, const IgemmKnobs& k) {
  if (k.policy != kDefaultPolicy || k.force_cfg >= 0) return {-1, 1};
  if (k.table_override >= 0 && q.epi == EPI_STORE && !q.lnf) {     // tuning: every plain-store launch as if the table held this entry
    const int sp = (k.table_override >> 8) & 0xff;
    return {k.table_override & 0xff, sp < 1 ? 1 : sp};
  }
  const int K = q.taps * (q.C0 + q.C1);
  for (const IgemmTuned* e = kIgemmTuned; e->dtype >= 0; ++e)
    if (e->M == q.M && e->N == q.N && e->K == K && e->dtype == dtype && e->taps == q.taps && e->stride == q.stride && e->up == q.up &&
        e->epi == q.epi && e->lnf == (q.lnf ? 1 : 0))
      return {e->cfg, e->splits};
  return {-1, 1};
}

// ---- the pieces every rule shares
constexpr int igemm_bke(int dtype) { return dtype == DT_BF16 ? 64 : 32; }     // K elements of one 128-byte K tile
// N tile of a launch: N is already padded, so the widest tile that divides it (igemm_pick_bn pads by the real N instead)
constexpr int igemm_n_tile(int N, int epi) { return epi == EPI_GEGLU ? 128 : N % 160 == 0 ? 160 : N % 128 == 0 ? 128 : N % 64 == 0 ? 64 : 32; }
constexpr long igemm_tiles(int M, int bm, int N, int bn) { return (long)((M + bm - 1) / bm) * (N / bn); }
constexpr int igemm_slices(int splits) { return splits > 1 ? splits : 1; }
// K tiles per slice (an extra tap's channels count where the launch has one)
constexpr int igemm_nk_slice(const IgemmLaunchDesc& q, int dtype, int splits) {
  return ((q.taps * (q.C0 + q.C1) + q.C2 + q.C3) / igemm_bke(dtype)) / igemm_slices(splits);
}
// 8-wave 128-row tile, one workgroup per CU (3-stage ring, pipelined K loop): the mid-size grids
// (16x16 / 32x32 feature maps) where 128-row tiles x K slices give about one work item per CU.  Versus
// two co-resident 64-row workgroups it stages 36% fewer operand bytes per FLOP through the LDS DMA.
constexpr bool igemm_mid8_ok(const IgemmKnobs& k, int cus, long t128, int splits) {
  const long items = t128 * igemm_slices(splits);
  return (k.policy & 16) && items >= 160 && items <= 2 * (long)cus;
}

// ---- what the engines ask before they build a launch
inline bool igemm_xt_ok_pure(const IgemmLaunchDesc& q, int dtype, const IgemmKnobs& k) {
  return k.xt_mode && dtype == DT_BF16 && q.C2 > 0 && q.C2 % 64 == 0 && q.C3 % 64 == 0 && q.taps == 9 && q.stride == 1 && !q.up && !q.cm &&
         q.N % 160 == 0 && q.epi == EPI_STORE && !q.lnf && k.policy == kDefaultPolicy && k.force_cfg < 0;
}
inline bool igemm_up4_ok_pure(const IgemmKnobs& k, long rows, int C, int N, int dtype) {
  return k.up4_mode && dtype == DT_BF16 && C % 64 == 0 && N % 160 == 0 && rows % 256 == 0 && k.policy == kDefaultPolicy && k.force_cfg < 0;
}
inline bool igemm_conv_cm_pure(const IgemmKnobs& k, int hw, int ctot, int n, int ksize, int stride, int up, int dtype) {
  if (ksize != 3 || stride != 1 || up || k.cm_mode == 0 || dtype != DT_BF16 || n % 160 != 0) return false;   // (what igemm_choose can run)
  return k.cm_mode == 1 || (hw >= 4096 && ctot >= 640);
}

// the checks of launch_igemm that the description carries (launch_igemm adds those on pointers and map geometry)
inline bool igemm_desc_ok(const IgemmLaunchDesc& q, int dtype, const IgemmKnobs& k) {
  const int bke = igemm_bke(dtype);
  const bool lnf = q.lnf != 0;
  if (q.M <= 0 || q.N <= 0 || q.N % 32 != 0 || q.C0 % bke != 0 || q.C1 % bke != 0 || (q.C0 + q.C1) == 0) return false;
  if (q.up4) {
    if (dtype != DT_BF16 || q.taps != 4 || q.stride != 1 || q.up || q.cm || q.C2 || q.epi != EPI_STORE || lnf || q.N % 160 != 0 || q.M % 1024 != 0)
      return false;
  } else if (q.taps != 1 && q.taps != 9) return false;
  if (q.cm && (q.taps != 9 || q.stride != 1 || q.up)) return false;
  if (q.epi == EPI_GEGLU && q.N % 128 != 0) return false;
  if (q.splits > 1 && q.epi != EPI_STORE) return false;
  if (lnf && (q.splits > 1 || (q.epi != EPI_STORE && q.epi != EPI_GEGLU))) return false;
  if ((q.C2 > 0 || q.C3 > 0) && !igemm_xt_ok_pure(q, dtype, k)) return false;
  return true;
}

// Split-K plan for grids that would leave most of the CUs idle (the 8x8 / 16x16 feature maps): the number of K slices
// (1 = no split), for the tile igemm_choose will take.
inline int igemm_plan_splits_pure(const IgemmLaunchDesc& q, int dtype, const IgemmKnobs& k, int cus) {
  if (q.epi != EPI_STORE || q.lnf || !igemm_desc_ok(q, dtype, k)) return 1;     // (nor for a launch igemm_choose will refuse)
  if (q.up4) {                 // 256-row tiles: K slices until every CU has a work item, at least 10 K tiles per slice
    const long t256 = igemm_tiles(q.M, 256, q.N, 160);
    const int nk0 = igemm_nk_slice(q, dtype, 1);
    int sp = t256 >= 240 ? 1 : (int)((cus + t256 / 2) / t256);
    if (sp > nk0 / 10) sp = nk0 / 10;
    if (sp > 8) sp = 8;
    return sp < 2 ? 1 : sp;
  }
  if (const IgemmTableHit e = igemm_table(q, dtype, k); e.cfg >= 0) return e.splits;
  const int bn = igemm_n_tile(q.N, q.epi);
  const long t128 = igemm_tiles(q.M, 128, q.N, bn);
  const int nk = q.taps * (q.C0 + q.C1) / igemm_bke(dtype);
  if ((k.policy & 16) && bn >= 128 && t128 < 200 && igemm_tiles(q.M, 256, q.N, bn) < 240) {
    // 128-row 8-wave tiles: aim at one work item per CU, at least 10 K tiles per slice (a 20-tile
    // K=1280 GEMM measured faster unsplit on 64-row tiles than split in two plus the finish pass)
    int sp = (int)((cus + t128 / 2) / t128);
    if (sp > nk / 10) sp = nk / 10;
    if (nk < 32) sp = 1;
    if (sp > 16) sp = 16;
    if (sp >= 2 && igemm_mid8_ok(k, cus, t128, sp)) return sp;
  }
  const long blocks = igemm_tiles(q.M, (bn >= 128 && t128 < 400) ? 64 : 128, q.N, bn);
  if (blocks >= 400 || nk < 24) return 1;
  int splits = (int)((512 + blocks - 1) / blocks);
  if (splits > nk / 12) splits = nk / 12;
  if (splits > 16) splits = 16;
  return splits < 2 ? 1 : splits;
}

// The form (index into kIgemmForms) and N tile of a launch that passed igemm_desc_ok; -2: no such launch.
inline int igemm_choose_form(const IgemmLaunchDesc& q, int dtype, const IgemmKnobs& k, int cus, int& bn) {
  const bool bf = dtype == DT_BF16, geglu = q.epi == EPI_GEGLU, lnf = q.lnf != 0;
  const int pol = k.policy, sp = igemm_slices(q.splits);
  bn = 160;
  // one tile form: 256 x 160 with loader waves (every up4 launch is >= 240 work items, K >= 20 tiles)
  if (q.up4) return bf ? 0 : -2;
  if (q.C2 > 0) {
    // conv2 + conv_shortcut of a resnet as one launch: the three tile forms the UNet's resnet convs use
    if (!bf || q.N % 160 != 0) return -2;
    const int cfg = igemm_table(q, DT_BF16, k).cfg;
    if (cfg == 0 || cfg == 3 || cfg == 4) return cfg;
    const long t256 = igemm_tiles(q.M, 256, q.N, 160);
    if (t256 >= 240) return 0;
    if (igemm_mid8_ok(k, cus, igemm_tiles(q.M, 128, q.N, 160), sp)) return igemm_nk_slice(q, dtype, sp) >= 40 ? 3 : 4;
    return t256 * sp >= 160 ? 0 : 3;
  }
  // channel-major 3x3 conv: one instantiation (the 256-row loader-wave tile the large maps use anyway), bf16 only
  if (q.cm) return bf && !lnf && q.epi == EPI_STORE && q.N % 160 == 0 ? 0 : -2;
  if (!q.x3) {             // a forced entry, or the launch table's
    const int cfg = k.force_cfg >= 0 ? k.force_cfg : igemm_table(q, dtype, k).cfg;
    bn = geglu ? 128 : (q.N % 160 == 0 ? 160 : (q.N % 128 == 0 ? 128 : 0));
    if (cfg >= 0 && cfg < kNumCfg && bn && igemm_form_exists(cfg, dtype, bn, lnf, false, false, false)) return cfg;
    if (k.force_cfg >= 0) return -2;     // a forced entry that does not exist for this launch is an error
  }
  bn = igemm_n_tile(q.N, q.epi);
  const long t256 = igemm_tiles(q.M, 256, q.N, bn), t128 = igemm_tiles(q.M, 128, q.N, bn), t64 = igemm_tiles(q.M, 64, q.N, bn);
  if (!bf && q.x3) {
    // split-bf16 mode: the arithmetic lives in the plain K loop only, so these launches take the plain-loop forms.
    // Tile choice: fp32 operands double the bytes staged per MAC, so these launches are bound by the L2 -> LDS path before the
    // split's VALU work: the largest tile wins even where its 64 x 80 wave tiles spill 17-19 VGPRs in this loop (measured:
    // 36.8 ms per B = 8 / L = 64 forward with the large tiles against 41.0 ms with spill-free 64-row tiles)
    if (bn < 128) return kNarrowForm;
    if (!lnf && t256 * sp >= 240) return 2;
    if (t128 * sp >= 400) return 8;
    return t64 * sp <= cus ? 6 : 7;
  }
  if (lnf) {
    // a folded LayerNorm (norm1 -> q|k|v, norm3 -> GEGLU: K = C <= 1280, N a multiple of 160 or GEGLU's 128): the rules below,
    // restricted to the forms those shapes can reach
    if (!geglu && q.N % 160 != 0) return -2;
    if (t256 >= 240) return geglu && (pol & 32) && bf ? 0 : 1;
    if (!geglu && igemm_mid8_ok(k, cus, t128, 1)) return 4;
    return t64 <= cus ? 6 : 7;
  }
  if (bn < 128) return kNarrowForm;
  // plenty of rows: 256-row tiles / 8 waves cut the operand bytes staged per FLOP (the K loop is
  // bound by global->LDS traffic, not by MFMA issue) as long as every CU still gets a workgroup
  // (the global->LDS path tops out near 12 TB/s chip-wide, i.e. needs ~70 KB in flight per CU).
  // One workgroup per CU then has to keep two tiles in flight itself: a 3-stage ring.
  const bool big = (pol & 1) && t256 >= 240;
  const int nk_slice = igemm_nk_slice(q, dtype, sp);
  if (!big && !geglu && igemm_mid8_ok(k, cus, t128, sp)) {
    // long K slices: 4 compute waves (64x80 each) + 4 loader waves, 4-stage ring - measured 3-15 % faster than the 8-wave
    // form on the >= 45-tile conv launches of the 16x16 / 32x32 maps and slower on short K (policy bit 1 turns it off)
    return !(pol & 2) && nk_slice >= 40 ? 3 : 4;
  }
  if (big) {
    // 256-row tiles with four extra loader waves (12-wave workgroups): issuing an LDS-DMA instruction parks the issuing wave
    // for 60-185 cycles (MI355X_MICROARCH.md), which in the 8-wave form comes straight out of the MFMA stream.  Measured on the
    // B = 8, L = 64 layer shapes (tools/kbench.py): 3x3 convs with K >= 2880 5-17 % faster, GEGLU 5-10 %, K <= 960 GEMMs 5-13 %
    // slower (prologue / epilogue bound: the loader waves only add barrier participants) -> long K slices and GEGLU only.
    // (bf16 only: the fp32 instantiation spills)
    if ((pol & 32) && bf && (nk_slice >= 24 || geglu)) return 0;
    return (pol & 8) ? 1 : 2;
  }
  // 128-row tiles that cannot put two workgroups on every CU: deeper ring, one workgroup per CU
  if ((pol & 2) && t128 >= 200 && t128 < 400) return 5;
  // fewer than ~1.5 workgroups per CU with 128-row tiles: halve the M tile (2 co-resident
  // workgroups per CU are what hides the per-K-tile barrier)
  if (t128 >= 400) return 8;
  // at most one workgroup per CU anyway: the DMA round trip (~1.1 us) is then hidden only by the
  // workgroup's own ring, so run it four stages deep instead of two
  return (pol & 4) && t64 * sp <= cus ? 6 : 7;
}

// The whole decision for one launch: 0 and *d filled, or -2 = no such launch.
inline int igemm_choose(const IgemmLaunchDesc& q, int dtype, const IgemmKnobs& k, int cus, IgemmDispatch* d) {
  if (!igemm_desc_ok(q, dtype, k)) return -2;
  int bn = 0;
  const int f = igemm_choose_form(q, dtype, k, cus, bn);
  const bool lnf = q.lnf != 0, cm = q.cm != 0, xt = q.C2 > 0;
  if (f < 0 || !igemm_form_exists(f, dtype, bn, lnf, cm, xt, q.up4 != 0)) return -2;
  const IgemmForm& t = kIgemmForms[f];
  const int sp = igemm_slices(q.splits), mt = (q.M + t.bm - 1) / t.bm, nt = q.N / bn, nwork = mt * nt * sp;
  // persistent grid: as many workgroups as fit on the chip at once (2 per CU for the 4-wave tiles,
  // 1 per CU for the 8-wave ones); each walks nwork / grid items
  const int resident = cus * ((t.wm * t.wn == 4 && t.nst == 2 && t.ldr == 0) ? 2 : 1);
  const int grid = nwork < resident ? nwork : resident;
  *d = IgemmDispatch{dtype == DT_BF16 ? DT_BF16 : DT_F32, t.bm, bn, t.wm, t.wn, t.nst, t.pipe ? 1 : 0, t.ldr, sp, grid, lnf ? 1 : 0, cm ? 1 : 0, 0,
                     xt ? 1 : 0, q.up4 ? 1 : 0, dtype == DT_BF16 ? 0 : q.x3, 0};
  // Cooperative finish inside the launch: every (tile, K slice) item has a workgroup of its own and all of them fit on the chip
  // together (one per CU is what every instantiation can hold), the slab set is addressable through one buffer descriptor,
  // the tile's counters fit the caller's region.  Otherwise: slabs + the finish kernel.
  // (measured per launch shape, tools/cf_bench.py: the in-launch finish wins 2-4 % on the 256-row tiles with 2-4 slices and loses
  // 2-20 % on the 128-row tiles with 8 - the serial chain drain -> ticket -> poll -> read costs what boundary + finish launch do;
  // mode bit 3 takes it on every tile form that has the instantiation)
  if (t.cf && dtype == DT_BF16 && bn == 160 && !lnf && !cm && (t.bm == 256 || (k.cf_mode & 8)) && q.splits > 1 && q.splits <= 32 && !q.no_finish && q.region &&
      (k.cf_mode & 1) && nwork == grid && nwork <= cus && (size_t)q.splits * q.M * q.N * sizeof(float) < ((size_t)1 << 31) &&
      (size_t)(2 * mt * nt + 2) * 8 <= kIgemmCfBytes) {
    const int us = (k.cf_mode >> 8) & 0xffff;
    d->cf = 1;
    d->cf_poll = (k.cf_mode & 2) ? 0 : (us ? us : 200) * 100;
  }
  return 0;
}

}  // namespace ldmseg
