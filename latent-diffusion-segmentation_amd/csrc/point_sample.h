// Taps of F.grid_sample(input, 2 * u - 1, align_corners=False, padding_mode='zeros') for one point u = (x, y) in [0, 1]^2 - what
// detectron2's point_sample (losses.py:168-178, :342-353) evaluates - in fp32 and in torch's own order of operations:
//   g   = 2 * u - 1                                        the grid torch is handed (2 * u is exact, one rounding)
//   pos = fma(g + 1, size / 2, -0.5)                       unnormalize of align_corners=False: torch's CPU kernel forms it with ONE
//                                                          rounding (size / 2 is exact); a separately rounded product picks other
//                                                          weights at sizes that are no power of two
//   bilinear  x0 = floor(pos), w = pos - x0, e = 1 - w     (likewise n, s in y); weights nw = s * e, ne = s * w, sw = n * e, se = n * w
//   nearest   nearbyint(pos): half to even
// A tap outside the map contributes 0 (zeros padding): with u < 1 that is column / row -1 and `size`.
// Pure: no state, usable on host and device; tests/test_point_loss_cpu.py checks it against torch through ldmseg_op_point_taps.
// Every product / difference is rounded separately (contraction off), the one fused step is spelled out.
#pragma once

#include <cmath>

namespace ldmseg {

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LDMSEG_HD __host__ __device__
#else
#define LDMSEG_HD
#endif

LDMSEG_HD inline float point_position(float u, int size) {
#pragma clang fp contract(off)
  const float g = 2.0f * u - 1.0f;
  return __builtin_fmaf(g + 1.0f, (float)size * 0.5f, -0.5f);
}

struct BilinearTaps {
  int x0, y0;                 // north-west tap; the others are (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1)
  float nw, ne, sw, se;
};

LDMSEG_HD inline BilinearTaps bilinear_taps(float ux, float uy, int H, int W) {
#pragma clang fp contract(off)
  const float ix = point_position(ux, W), iy = point_position(uy, H);
  const float fx = floorf(ix), fy = floorf(iy);
  const float w = ix - fx, e = 1.0f - w, n = iy - fy, s = 1.0f - n;
  BilinearTaps t;
  t.x0 = (int)fx; t.y0 = (int)fy;
  t.nw = s * e; t.ne = s * w; t.sw = n * e; t.se = n * w;
  return t;
}

LDMSEG_HD inline bool tap_inside(int x, int y, int H, int W) { return x >= 0 && x < W && y >= 0 && y < H; }

// linear index y * W + x of the nearest tap, -1 outside the map
LDMSEG_HD inline int nearest_tap(float ux, float uy, int H, int W) {
  const float ix = point_position(ux, W), iy = point_position(uy, H);
  const int x = (int)nearbyintf(ix), y = (int)nearbyintf(iy);
  return tap_inside(x, y, H, W) ? y * W + x : -1;
}

// bilinear sample of one fp32 plane [H][W]: torch adds the four products in the order nw, ne, sw, se
template <typename Load>
LDMSEG_HD inline float bilinear_sample(const BilinearTaps& t, int H, int W, Load load) {
#pragma clang fp contract(off)
  const bool x0 = t.x0 >= 0 && t.x0 < W, x1 = t.x0 + 1 >= 0 && t.x0 + 1 < W;
  const bool y0 = t.y0 >= 0 && t.y0 < H, y1 = t.y0 + 1 >= 0 && t.y0 + 1 < H;
  float v = 0.0f;
  if (x0 && y0) v = load(t.y0 * W + t.x0) * t.nw;
  if (x1 && y0) v = v + load(t.y0 * W + t.x0 + 1) * t.ne;
  if (x0 && y1) v = v + load((t.y0 + 1) * W + t.x0) * t.sw;
  if (x1 && y1) v = v + load((t.y0 + 1) * W + t.x0 + 1) * t.se;
  return v;
}

#undef LDMSEG_HD

}  // namespace ldmseg
