// Which launch a conv / transposed-conv weight gradient (launch_wgrad, vae_bwd.hip) runs: the tile, the slicing of the pixel axis
// and the grid (wgrad_choose).  Plain C++17: no HIP, no state - a function of the launch description and the CU count, so it runs
// (and is tested, tests/test_wgrad_plan_cpu.py) without a device.
//
// The GEMM: dW[n][tap][c] = sum over pixels p of dY[p][n] * X[p + tap][c].  The contraction runs over the pixels (hundreds of
// thousands), the output is tiny, so the parallelism comes from slicing the pixel axis.  Every slice writes its own slab
// [slice][N][taps * C]; wgrad_finish adds the slabs in slice order.  The slicing - and with it the order of every addition - is
// a function of the SHAPE alone: it aims at kWgradTargetItems work items whatever the device; the CU count only decides how many
// workgroups walk the items (one item per workgroup while they fit, a fixed-stride walk beyond).
//
// Two rules share one body (WgradRule).  The decoder's: the 128 x 128 tile, stride 1.  The encoder's: dY
// lives on the OUTPUT map of a stride-1 or stride-2 conv, and the tile follows the storage widths - 32, 64 or 128 rows of dY by 32,
// 64 or 128 channels of X - so that a 32- or 64-channel layer does not pay for a 128-wide tile.
#pragma once
#include <cstdio>
#include <string>

namespace ldmseg {

// P pixels of the map dY lives on (the OUTPUT map of a conv of stride 1 | 2; stride 1: the map X lives on too), N rows of dY taken
// (storage width of dY), C storage channels of X, taps 9 (3x3, pad 1) or 1, x3: 0 = exact fp32 MFMA, 1 = split-bf16 products,
// stride 2: taps 9 only
struct WgradDesc { int P, N, C, taps, x3, stride = 1; };
enum WgradRule {
  kWgradFixedTile = 0,   // the decoder's: the 128 x 128 tile per tap, stride 1
  kWgradByWidth = 1,     // the encoder's: the tile follows N and C; all nine taps in one workgroup where both fit 64
};
// side of the output map of a 3x3 conv, pad 1, on a side of h pixels (odd h included)
constexpr int conv_out_dim(int h, int stride) { return stride == 2 ? (h - 1) / 2 + 1 : h; }

constexpr int kWgradTileN = 128, kWgradTileC = 128;   // output tile of a workgroup: four waves of 64 x 64
constexpr int kWgradStep = 32;                          // pixels per K step (one bf16 MFMA's K; eight fp32 MFMAs' K)
constexpr int kWgradMinSteps = 8;                       // a slice is worth a workgroup from 256 pixels on
constexpr int kWgradTargetItems = 256;                  // work items the slicing aims at (the CU count of an MI355X)

struct WgradPlan {
  int x3 = 0;
  int tile_n = kWgradTileN, tile_c = kWgradTileC;       // output tile of a workgroup (per tap): 2 x 2 waves of tile_n/2 x tile_c/2
  int stride = 1;
  int n_tiles = 1, c_tiles = 1, taps = 1, tiles = 1;    // tiles = n_tiles * c_tiles * taps (all_taps: n_tiles * c_tiles)
  int all_taps = 0;                                     // a workgroup owns the nine taps of its tile: tile_n x 9 tile_c outputs
  int steps = 1;                                        // K steps over all pixels
  int slices = 1, steps_per_slice = 1;                  // slice s takes steps [s * steps_per_slice, min(steps, (s + 1) * steps_per_slice))
  int items = 1;                                        // tiles * slices
  int grid_x = 1, block = 256;
  int one_per_cu = 1;                                   // every item has its own workgroup (grid_x == items <= CUs)
};

// the narrowest of 32 | 64 | 128 that holds `width` (128 beyond)
constexpr int wgrad_tile_for(int width) { return width <= 32 ? 32 : width <= 64 ? 64 : 128; }

// 0 and *out filled, or -2: no such launch.
// By width, a 3x3 layer whose two widths fit 64 runs on the all-taps tile: one workgroup owns N x 9 C outputs of a slice, reads dY
// once per step and X with its halo, so the operand traffic does not scale with the tap count (and the slicing aims at 256 slices,
// not 28).
inline int wgrad_choose(const WgradDesc& q, WgradRule rule, int cus, WgradPlan* out) {
  if (q.P < 1 || q.N < 1 || q.C < 1 || (q.taps != 1 && q.taps != 9) || cus < 1) return -2;
  if (q.stride != 1 && (rule != kWgradByWidth || q.stride != 2 || q.taps != 9)) return -2;
  if (q.N % 16 || q.C % 16) return -2;                  // operands are read as 16-channel MFMA fragments
  if ((long long)q.P + 2 * kWgradStep >= (1ll << 31)) return -2;
  const bool by_width = rule == kWgradByWidth;
  WgradPlan p;
  p.x3 = q.x3 ? 1 : 0;
  p.taps = q.taps;
  p.stride = q.stride;
  p.tile_n = by_width ? wgrad_tile_for(q.N) : kWgradTileN;
  p.tile_c = by_width ? wgrad_tile_for(q.C) : kWgradTileC;
  p.n_tiles = (q.N + p.tile_n - 1) / p.tile_n;
  p.c_tiles = (q.C + p.tile_c - 1) / p.tile_c;
  p.all_taps = by_width && q.taps == 9 && p.tile_n <= 64 && p.tile_c <= 64 ? 1 : 0;
  p.tiles = p.n_tiles * p.c_tiles * (p.all_taps ? 1 : p.taps);
  p.steps = (q.P + kWgradStep - 1) / kWgradStep;
  int want = kWgradTargetItems / p.tiles;               // slices that fill the target
  const int worth = p.steps / kWgradMinSteps;           // slices the pixel axis is worth
  if (want > worth) want = worth;
  if (want < 1) want = 1;
  p.steps_per_slice = (p.steps + want - 1) / want;
  p.slices = (p.steps + p.steps_per_slice - 1) / p.steps_per_slice;   // no empty slice
  p.items = p.tiles * p.slices;
  p.one_per_cu = p.items <= cus ? 1 : 0;
  p.grid_x = p.one_per_cu ? p.items : cus;
  *out = p;
  return 0;
}
// MACs a plan executes for one pixel: tiles x tile area x taps (the chooser's cost, tests/test_wgrad_plan_ex_cpu.py)
inline long long wgrad_plan_macs_per_pixel(const WgradPlan& p) { return (long long)p.n_tiles * p.c_tiles * p.taps * p.tile_n * p.tile_c; }

inline std::string wgrad_plan_name(const WgradPlan& p) {
  char b[64];
  std::snprintf(b, sizeof b, "wgrad%s<%s,%d,%d>/taps%d%s", p.all_taps ? "9" : "", p.x3 ? "x3" : "f32", p.tile_n, p.tile_c, p.taps,
                p.stride == 2 ? "/s2" : "");
  return b;
}
// "name tiles=T slices=S steps=K/slice grid=G block=256 one_per_cu=0|1"
inline std::string wgrad_plan_line(const WgradPlan& p) {
  char b[128];
  std::snprintf(b, sizeof b, " tiles=%d slices=%d steps=%d/%d grid=%d block=%d one_per_cu=%d", p.tiles, p.slices, p.steps_per_slice,
                p.steps, p.grid_x, p.block, p.one_per_cu);
  return wgrad_plan_name(p) + b;
}

}  // namespace ldmseg
