// What both directions of the stage-1 point loss evaluate per point (point_loss.hip forward, point_loss_bwd.hip backward): the
// row table, the effective target under the validity mask, which draw a point is (one of the kU selected oversampled draws or a
// fresh one), the cross-entropy point (nearest-tap label, logits / T, running maximum and fp64 sum of exponentials) and the mask
// point (bilinear logit, bilinear target, sigmoid).  Written once here so that the gradient is taken at exactly the points, labels
// and targets the forward value was computed from.  Device code, included by files compiled with -ffp-contract=off.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "point_sample.h"
#include "reduce_dev.h"

namespace ldmseg {
namespace pointloss {

constexpr int kThreads = 256;
static_assert(kThreads == kBlockSumThreads, "block_sum (reduce_dev.h) sums kBlockSumThreads / 64 waves");

// effective target of pixel i of image b: the masked pixels count as ignore_label (losses.py:326, without touching the caller's tensor)
__device__ __forceinline__ int64_t eff_target(const PointLoss& p, int b, int i) {
  const size_t at = (size_t)b * p.Ht * p.Wt + i;
  if (p.valid && !p.valid[at]) return p.ignore;
  return p.tgt[at];
}

// ---------------------------------------------------------------- rows
struct Row {
  int b, c;                  // c < 0: the cross-entropy row of image b
  const float* over;         // [S][2] or null
  const float* fresh;        // [P - kU][2]
};
__device__ __forceinline__ Row row_of(const PointLoss& p, int r) {
  Row w;
  if (r < p.B) {
    w.b = r; w.c = -1;
    w.over = p.ce_over ? p.ce_over + (size_t)r * p.S * 2 : nullptr;
    w.fresh = p.ce_fresh ? p.ce_fresh + (size_t)r * (p.P - p.kU) * 2 : nullptr;
  } else {
    const int m = r - p.B;
    const int bc = p.rows[m];
    w.b = bc / p.C; w.c = bc - w.b * p.C;
    w.over = p.m_over ? p.m_over + (size_t)m * p.S * 2 : nullptr;
    w.fresh = p.m_fresh ? p.m_fresh + (size_t)m * (p.P - p.kU) * 2 : nullptr;
  }
  return w;
}

// point j of row r: the first kU are the selected oversampled draws (in index order), the rest the fresh ones
struct PointUV {
  float x, y;
};
__device__ __forceinline__ PointUV point_uv(const PointLoss& p, const Row& w, int r, int j) {
  PointUV u;
  if (j < p.kU) {
    int i = p.sel[(size_t)r * p.kU + j];
    i = i < 0 ? 0 : (i >= p.S ? p.S - 1 : i);
    u.x = w.over[2 * i]; u.y = w.over[2 * i + 1];
  } else {
    u.x = w.fresh[2 * (j - p.kU)]; u.y = w.fresh[2 * (j - p.kU) + 1];
  }
  return u;
}

// ---------------------------------------------------------------- cross-entropy point
// logit of channel plane xc at the taps t, divided by the temperature
__device__ __forceinline__ float ce_logit(const PointLoss& p, const BilinearTaps& t, const float* xc) {
#pragma clang fp contract(off)
  return __fdiv_rn(bilinear_sample(t, p.H, p.W, [&](int i) { return xc[i]; }), p.temperature);
}

struct CePoint {
  bool kept;                 // label != ignore_label
  int64_t label;
  float mx, at_label;        // max_c z_c and z_label, z = x / T
  double sum;                // sum_c exp(z_c - mx)
};
__device__ __forceinline__ CePoint ce_point(const PointLoss& p, const Row& w, const PointUV& u, const BilinearTaps& t) {
#pragma clang fp contract(off)
  CePoint q;
  // grid_sample(mode='nearest') of the float target map with zeros padding: outside the map the label is 0
  const int ti = nearest_tap(u.x, u.y, p.Ht, p.Wt);
  q.label = ti < 0 ? 0 : eff_target(p, w.b, ti);
  q.kept = q.label != p.ignore;
  q.mx = -INFINITY; q.at_label = 0.0f; q.sum = 0.0;
  if (!q.kept) return q;
  const size_t plane = (size_t)p.H * p.W;
  const float* xb = p.x + (size_t)w.b * p.C * plane;
  for (int c = 0; c < p.C; ++c) {
    const float v = ce_logit(p, t, xb + (size_t)c * plane);
    q.mx = fmaxf(q.mx, v);
    if (c == q.label) q.at_label = v;
  }
  for (int c = 0; c < p.C; ++c) {
    const float v = ce_logit(p, t, xb + (size_t)c * plane);
    q.sum += (double)expf(v - q.mx);
  }
  return q;
}

// ---------------------------------------------------------------- mask point
struct MaskPoint {
  float x, y, sg;            // bilinear logit, bilinear sample of (effective target == c), sigmoid(x)
};
__device__ __forceinline__ MaskPoint mask_point(const PointLoss& p, const Row& w, const PointUV& u, const BilinearTaps& t) {
#pragma clang fp contract(off)
  MaskPoint q;
  const float* xc = p.x + ((size_t)w.b * p.C + w.c) * ((size_t)p.H * p.W);
  q.x = bilinear_sample(t, p.H, p.W, [&](int i) { return xc[i]; });
  const BilinearTaps tt = bilinear_taps(u.x, u.y, p.Ht, p.Wt);
  const int64_t cls = w.c;
  q.y = bilinear_sample(tt, p.Ht, p.Wt, [&](int i) { return eff_target(p, w.b, i) == cls ? 1.0f : 0.0f; });
  q.sg = 1.0f / (1.0f + expf(-q.x));
  return q;
}

inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

}  // namespace pointloss
}  // namespace ldmseg
