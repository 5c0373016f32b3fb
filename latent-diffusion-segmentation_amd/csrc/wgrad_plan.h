// Which launch a conv / transposed-conv weight gradient (launch_wgrad, vae_bwd.hip) runs: the tile, the slicing of the pixel axis
// and the grid (wgrad_choose).  Plain C++17: no HIP, no state - a function of the launch description and the CU count, so it runs
// (and is tested, tests/test_wgrad_plan_cpu.py) without a device.
//
// The GEMM: dW[n][tap][c] = sum over pixels p of dY[p][n] * X[p + tap][c].  The contraction runs over the pixels (hundreds of
// thousands), the output is tiny, so the parallelism comes from slicing the pixel axis.  Every slice writes its own slab
// [slice][N][taps * C]; wgrad_finish adds the slabs in slice order.  The slicing - and with it the order of every addition - is
// a function of the SHAPE alone: it aims at kWgradTargetItems work items whatever the device; the CU count only decides how many
// workgroups walk the items (one item per workgroup while they fit, a fixed-stride walk beyond).
#pragma once
#include <cstdio>
#include <string>

namespace ldmseg {

// P pixels (B * H * W of the map X lives on), N rows of dY taken (storage width of dY), C storage channels of X, taps 9 (3x3, pad
// 1) or 1, x3: 0 = exact fp32 MFMA, 1 = split-bf16 products
struct WgradDesc { int P, N, C, taps, x3; };

constexpr int kWgradTileN = 128, kWgradTileC = 128;   // output tile of a workgroup: four waves of 64 x 64
constexpr int kWgradStep = 32;                          // pixels per K step (one bf16 MFMA's K; eight fp32 MFMAs' K)
constexpr int kWgradMinSteps = 8;                       // a slice is worth a workgroup from 256 pixels on
constexpr int kWgradTargetItems = 256;                  // work items the slicing aims at (the CU count of an MI355X)

struct WgradPlan {
  int x3 = 0;
  int n_tiles = 1, c_tiles = 1, taps = 1, tiles = 1;    // tiles = n_tiles * c_tiles * taps
  int steps = 1;                                        // K steps over all pixels
  int slices = 1, steps_per_slice = 1;                  // slice s takes steps [s * steps_per_slice, min(steps, (s + 1) * steps_per_slice))
  int items = 1;                                        // tiles * slices
  int grid_x = 1, block = 256;
  int one_per_cu = 1;                                   // every item has its own workgroup (grid_x == items <= CUs)
};

// 0 and *out filled, or -2: no such launch
inline int wgrad_choose(const WgradDesc& q, int cus, WgradPlan* out) {
  if (q.P < 1 || q.N < 1 || q.C < 1 || (q.taps != 1 && q.taps != 9) || cus < 1) return -2;
  if (q.N % 16 || q.C % 16) return -2;                  // operands are read as 16-channel MFMA fragments
  if ((long long)q.P + 2 * kWgradStep >= (1ll << 31)) return -2;
  WgradPlan p;
  p.x3 = q.x3 ? 1 : 0;
  p.taps = q.taps;
  p.n_tiles = (q.N + kWgradTileN - 1) / kWgradTileN;
  p.c_tiles = (q.C + kWgradTileC - 1) / kWgradTileC;
  p.tiles = p.n_tiles * p.c_tiles * p.taps;
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

inline std::string wgrad_plan_name(const WgradPlan& p) {
  char b[64];
  std::snprintf(b, sizeof b, "wgrad<%s,%d,%d>/taps%d", p.x3 ? "x3" : "f32", kWgradTileN, kWgradTileC, p.taps);
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
