// Backward of the seg-VAE's stage-1 loss (point_loss.hip) to the logits x [B,C,H,W], and of posterior.kl() to the moments.
// Coordinates, the uncertainty selection, labels and targets carry no gradient (the reference computes them under no_grad); the
// one differentiable path is the bilinear sample of x at the chosen points, so the whole backward is a scatter of point gradients
// through their taps into a dense gradient.  Every point is evaluated by the forward's own code (point_loss_dev.h).
//
//   points   a thread per point, like point_loss_kernel: CE rows keep {max, 1 / sum of exponentials, label}, mask rows {logit,
//            target}; fp64 partials per workgroup for the kept points K and each mask row's sum(s t), sum(s), sum(t); an integer
//            atomic per tap inside the map counts the taps of every pixel.  Dropped CE points have no taps.
//   scan     a workgroup per image turns the counts into list starts; one more workgroup adds the partials in a fixed order.
//   fill     a thread per point again: every tap is stored ONCE into its pixel's list (an integer atomic hands out the slot):
//            key (row * P + point) * 4 + tap in the high word, and for mask rows the finished contribution coef * weight in the
//            low word.  A CE tap has one value per channel, which the last pass recomputes.
//   gather   a thread per pixel, the channel loop inside (lanes over pixels store whole lines of a plane; see point_loss.hip on
//            lanes over channels): sorts its list by key - slots were handed out in arrival order, the keys are unique - and adds
//            it in that order, 16 channels at a time in registers: first the CE taps (softmax_c from the saved max and 1 / sum and a
//            bilinear sample of plane c), then the taps of mask row (b, c).  Writes every element of grad_x once, 0.0 where the
//            list is empty.
//
// No float atomics: each float sum is a list in a fixed order, so two calls agree bit for bit.  Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/ldmseg_hip.h"
#include "common.h"
#include "kernels.h"
#include "point_loss_dev.h"
#include "point_sample.h"

namespace ldmseg {
namespace {

using namespace pointloss;

constexpr int kChunk = 16;     // channels a gather thread accumulates in registers per walk over its list

// weight and linear pixel index of tap k (0 nw, 1 ne, 2 sw, 3 se); -1 outside the map
__device__ __forceinline__ float tap_weight(const BilinearTaps& t, int k) { return k == 0 ? t.nw : (k == 1 ? t.ne : (k == 2 ? t.sw : t.se)); }
__device__ __forceinline__ int tap_pixel(const BilinearTaps& t, int k, int H, int W) {
  const int x = t.x0 + (k & 1), y = t.y0 + (k >> 1);
  return tap_inside(x, y, H, W) ? y * W + x : -1;
}

// does row r take part: a null upstream gradient leaves that term's rows out
__device__ __forceinline__ bool row_active(const PointLossGrad& g, int r) { return r < g.f.B ? g.g_ce != nullptr : g.g_mask != nullptr; }

// ---------------------------------------------------------------- points
// partial[(r * nchunk + chunk) * 4 + k]: CE rows {-, kept points, -, -}; mask rows {-, sigmoid * t, sigmoid, t} (the forward's slots)
__global__ __launch_bounds__(kThreads) void point_grad_points_kernel(const PointLossGrad g) {
#pragma clang fp contract(off)
  __shared__ double s_red[kThreads / 64];
  const PointLoss& p = g.f;
  const int r = blockIdx.y;
  const int j = blockIdx.x * kThreads + threadIdx.x;
  const Row w = row_of(p, r);
  const bool active = row_active(g, r);
  double a1 = 0.0, a2 = 0.0, a3 = 0.0;
  if (active && j < p.P) {
    const PointUV u = point_uv(p, w, r, j);
    const BilinearTaps t = bilinear_taps(u.x, u.y, p.H, p.W);
    const size_t at = (size_t)r * p.P + j;
    bool taps = true;
    if (w.c < 0) {
      const CePoint q = ce_point(p, w, u, t);
      g.rec_a[at] = q.mx;
      g.rec_b[at] = q.kept ? (float)(1.0 / q.sum) : 0.0f;
      // -1: dropped; an id outside [0, C) (the forward's caller refuses those) matches no channel
      g.rec_label[at] = !q.kept ? -1 : ((q.label >= 0 && q.label < p.C) ? (int32_t)q.label : p.C);
      a1 = q.kept ? 1.0 : 0.0;
      taps = q.kept;
    } else {
      const MaskPoint q = mask_point(p, w, u, t);
      g.rec_a[at] = q.x;
      g.rec_b[at] = q.y;
      const double sg = (double)q.sg, yd = (double)q.y;
      a1 = sg * yd; a2 = sg; a3 = yd;
    }
    if (taps) {
      int32_t* cnt = g.count + (size_t)w.b * p.H * p.W;
      for (int k = 0; k < 4; ++k) {
        const int px = tap_pixel(t, k, p.H, p.W);
        if (px >= 0) atomicAdd(cnt + px, 1);
      }
    }
  }
  const double t1 = block_sum(a1, s_red), t2 = block_sum(a2, s_red), t3 = block_sum(a3, s_red);
  if (threadIdx.x == 0) {
    double* q = g.f.partial + ((size_t)r * gridDim.x + blockIdx.x) * 4;
    q[0] = 0.0; q[1] = t1; q[2] = t2; q[3] = t3;
  }
}

// ---------------------------------------------------------------- scan
// workgroups 0 .. B-1: exclusive scan of image b's tap counts -> cursor (list starts, relative to the image's region of `entries`),
// and the region's start img_base[b] = 4 P (rows of the images before b): room for every tap of every row.
// workgroup B: stat[0] = K, stat[1 + 3 m ..] = {sum(s t), sum(s), sum(t)} of mask row m, partials added in chunk order.
__global__ __launch_bounds__(kThreads) void point_grad_scan_kernel(const PointLossGrad g, int nchunk) {
  __shared__ double s_red[kThreads / 64];
  __shared__ int s_run[kThreads];
  const PointLoss& p = g.f;
  if ((int)blockIdx.x == p.B) {
    double cnt = 0.0;
    for (int i = threadIdx.x; i < p.B * nchunk; i += kThreads) cnt += p.partial[(size_t)i * 4 + 1];
    const double cnt_t = block_sum(cnt, s_red);
    if (threadIdx.x == 0) g.stat[0] = cnt_t;
    for (int m = threadIdx.x; m < p.N; m += kThreads) {
      double a1 = 0.0, a2 = 0.0, a3 = 0.0;
      const double* q = p.partial + (size_t)(p.B + m) * nchunk * 4;
      for (int c = 0; c < nchunk; ++c) { a1 += q[4 * c + 1]; a2 += q[4 * c + 2]; a3 += q[4 * c + 3]; }
      g.stat[1 + 3 * m] = a1; g.stat[2 + 3 * m] = a2; g.stat[3 + 3 * m] = a3;
    }
    return;
  }
  const int b = blockIdx.x;
  const int n = p.H * p.W;
  const int32_t* cnt = g.count + (size_t)b * n;
  int32_t* cur = g.cursor + (size_t)b * n;
  const int seg = (n + kThreads - 1) / kThreads;
  const int lo = min(n, (int)threadIdx.x * seg), hi = min(n, lo + seg);
  int run = 0;
  for (int i = lo; i < hi; ++i) run += cnt[i];
  s_run[threadIdx.x] = run;
  __syncthreads();
  if (threadIdx.x == 0) {
    int acc = 0;
    for (int t = 0; t < kThreads; ++t) { const int v = s_run[t]; s_run[t] = acc; acc += v; }
    int before = 0;                                  // mask rows of the images before b (rows are ordered by image)
    for (int m = 0; m < p.N; ++m) before += p.rows[m] < b * p.C;
    g.img_base[b] = 4 * p.P * (b + before);
  }
  __syncthreads();
  run = s_run[threadIdx.x];
  for (int i = lo; i < hi; ++i) { cur[i] = run; run += cnt[i]; }
}

// ---------------------------------------------------------------- fill
__global__ __launch_bounds__(kThreads) void point_grad_fill_kernel(const PointLossGrad g) {
#pragma clang fp contract(off)
  const PointLoss& p = g.f;
  const int r = blockIdx.y;
  const int j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= p.P || !row_active(g, r)) return;
  const Row w = row_of(p, r);
  const size_t at = (size_t)r * p.P + j;
  float coef = 0.0f;
  if (w.c < 0) {
    if (g.rec_label[at] < 0) return;                 // a dropped point: no taps were counted
  } else {
    // d mask / d l of this point, times the upstream gradient
    const double* st = g.stat + 1 + 3 * (size_t)(r - p.B);
    const double I = st[0], D1 = (st[1] + st[2]) + 1.0;
    const float l = g.rec_a[at];
    const double t = (double)g.rec_b[at];
    const double s = (double)(1.0f / (1.0f + expf(-l)));
    const double bce = (s - t) / (double)p.P;
    const double dice = -((2.0 * t * D1 - (2.0 * I + 1.0)) / (D1 * D1)) * (s * (1.0 - s));
    coef = (float)((bce + dice) / g.num_masks) * g.g_mask[0];
  }
  const PointUV u = point_uv(p, w, r, j);
  const BilinearTaps t = bilinear_taps(u.x, u.y, p.H, p.W);
  int32_t* cur = g.cursor + (size_t)w.b * p.H * p.W;
  unsigned long long* e = g.entries + g.img_base[w.b];
  for (int k = 0; k < 4; ++k) {
    const int px = tap_pixel(t, k, p.H, p.W);
    if (px < 0) continue;
    const int slot = atomicAdd(cur + px, 1);         // afterwards cursor[px] is the END of the pixel's list
    const unsigned long long key = (unsigned long long)(uint32_t)((int)at * 4 + k);
    e[slot] = (key << 32) | (unsigned long long)__float_as_uint(coef * tap_weight(t, k));
  }
}

// ---------------------------------------------------------------- gather
__global__ __launch_bounds__(kThreads) void point_grad_gather_kernel(const PointLossGrad g) {
#pragma clang fp contract(off)
  const PointLoss& p = g.f;
  const int b = blockIdx.y;
  const int n = p.H * p.W;
  const int px = blockIdx.x * kThreads + threadIdx.x;
  if (px >= n) return;
  const int len = g.count[(size_t)b * n + px];
  unsigned long long* e = g.entries + g.img_base[b] + (g.cursor[(size_t)b * n + px] - len);
  // this thread alone owns the list: order it by key (row, point, tap)
  for (int i = 1; i < len; ++i) {
    const unsigned long long v = e[i];
    int k = i;
    for (; k > 0 && e[k - 1] > v; --k) e[k] = e[k - 1];
    e[k] = v;
  }
  // the CE taps (rows < B, so keys below 4 B P) come first, then the mask rows of this image by ascending class id
  const unsigned long long ce_end = (unsigned long long)p.B * p.P * 4;
  int nce = 0;
  while (nce < len && (e[nce] >> 32) < ce_end) ++nce;
  float scale = 0.0f;                                // g_ce / (T K); no kept point: 0, not 1 / 0
  if (g.g_ce && g.stat[0] > 0.0) scale = (float)(((double)g.g_ce[0] / g.stat[0]) / (double)p.temperature);
  auto class_of = [&](int i) -> int {
    if (i >= len) return 0x7fffffff;
    const int r = (int)((e[i] >> 34) / (unsigned long long)p.P);
    return p.rows[r - p.B] - b * p.C;
  };
  int mcur = nce, mc = class_of(mcur);
  const size_t plane = (size_t)n;
  const float* xb = p.x + (size_t)b * p.C * plane;
  float* gb = g.grad_x + (size_t)b * p.C * plane;
  const Row w = row_of(p, b);                        // the cross-entropy row of image b
  for (int c0 = 0; c0 < p.C; c0 += kChunk) {
    float acc[kChunk];
#pragma unroll
    for (int cc = 0; cc < kChunk; ++cc) acc[cc] = 0.0f;
    for (int i = 0; i < nce; ++i) {
      const int key = (int)(e[i] >> 32);
      const int at = key >> 2, k = key & 3;
      const PointUV u = point_uv(p, w, b, at - b * p.P);
      const BilinearTaps t = bilinear_taps(u.x, u.y, p.H, p.W);
      const float wk = tap_weight(t, k);
      const float mx = g.rec_a[at], inv = g.rec_b[at];
      const int label = g.rec_label[at];
#pragma unroll
      for (int cc = 0; cc < kChunk; ++cc) {
        const int c = c0 + cc;
        if (c < p.C) {
          const float v = ce_logit(p, t, xb + (size_t)c * plane);
          const float pr = expf(v - mx) * inv;
          acc[cc] = acc[cc] + ((pr - (c == label ? 1.0f : 0.0f)) * scale) * wk;
        }
      }
    }
#pragma unroll
    for (int cc = 0; cc < kChunk; ++cc) {
      const int c = c0 + cc;
      if (c < p.C) {
        while (mc == c) {
          acc[cc] = acc[cc] + __uint_as_float((uint32_t)e[mcur]);
          ++mcur;
          mc = class_of(mcur);
        }
        gb[(size_t)c * plane + px] = acc[cc];
      }
    }
  }
}

// ---------------------------------------------------------------- KL
// d kl_b / d mean = mean, d kl_b / d logvar = 0.5 (exp(logvar) - 1) where the clamp to [-30, 20] passes gradient (bounds included)
__global__ __launch_bounds__(kThreads) void gaussian_kl_backward_kernel(const float* moments, int n, const float* grad_per_image,
                                                                        float* grad_moments) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= 2 * n) return;
  const size_t at = (size_t)b * 2 * n + i;
  const float gb = grad_per_image[b];
  const float v = moments[at];
  float out;
  if (i < n) out = gb * v;
  else out = (v >= -30.0f && v <= 20.0f) ? (0.5f * gb) * (expf(v) - 1.0f) : 0.0f;
  grad_moments[at] = out;
}


// scratch layout of launch_point_loss_backward (bytes): partials | stat | rec_a | rec_b | rec_label | count | cursor | img_base | entries
struct GradScratch {
  size_t partial, stat, rec_a, rec_b, rec_label, count, cursor, img_base, entries, total;
};
inline GradScratch grad_scratch(int B, int HW, int N, int P) {
  GradScratch l;
  const size_t rows = (size_t)B + N, nchunk = (size_t)(P + kThreads - 1) / kThreads, pts = rows * P, pix = (size_t)B * HW;
  l.partial = 0;
  l.stat = up16(l.partial + rows * nchunk * 4 * sizeof(double));
  l.rec_a = up16(l.stat + (1 + 3 * (size_t)N) * sizeof(double));
  l.rec_b = up16(l.rec_a + pts * sizeof(float));
  l.rec_label = up16(l.rec_b + pts * sizeof(float));
  l.count = up16(l.rec_label + (size_t)B * P * sizeof(int32_t));
  l.cursor = up16(l.count + pix * sizeof(int32_t));
  l.img_base = up16(l.cursor + pix * sizeof(int32_t));
  l.entries = up16(l.img_base + (size_t)B * sizeof(int32_t));
  l.total = up16(l.entries + pts * 4 * sizeof(unsigned long long));
  return l;
}

}  // namespace

size_t point_loss_backward_scratch_bytes(int B, int C, int H, int W, int N, int kU, int P) {
  if (B < 1 || C < 1 || H < 1 || W < 1 || N < 0 || kU < 0 || P < 1 || (int64_t)H * W > (int64_t)0x7fff0000 ||
      ((int64_t)B + N) * P > (int64_t)0x1fff0000)
    return 0;
  return grad_scratch(B, H * W, N, P).total;
}

int launch_point_loss_backward(const PointLossGrad& in, void* scratch, hipStream_t s) {
  PointLossGrad g = in;                              // (arguments are checked by ldmseg_point_loss_backward, the one caller)
  const PointLoss& p = g.f;
  const int rows = p.B + p.N, HW = p.H * p.W;
  const GradScratch l = grad_scratch(p.B, HW, p.N, p.P);
  char* sc = (char*)scratch;
  g.f.partial = (double*)(sc + l.partial);
  g.stat = (double*)(sc + l.stat);
  g.rec_a = (float*)(sc + l.rec_a);
  g.rec_b = (float*)(sc + l.rec_b);
  g.rec_label = (int32_t*)(sc + l.rec_label);
  g.count = (int32_t*)(sc + l.count);
  g.cursor = (int32_t*)(sc + l.cursor);
  g.img_base = (int32_t*)(sc + l.img_base);
  g.entries = (unsigned long long*)(sc + l.entries);
  const int nchunk = (p.P + kThreads - 1) / kThreads;
  if (hipMemsetAsync(g.count, 0, (size_t)p.B * HW * sizeof(int32_t), s) != hipSuccess) return -3;
  LDMSEG_LAUNCH("point_grad_points", point_grad_points_kernel, dim3(nchunk, rows), dim3(kThreads), 0, s, g);
  LDMSEG_LAUNCH("point_grad_scan", point_grad_scan_kernel, dim3(p.B + 1), dim3(kThreads), 0, s, g, nchunk);
  LDMSEG_LAUNCH("point_grad_fill", point_grad_fill_kernel, dim3(nchunk, rows), dim3(kThreads), 0, s, g);
  LDMSEG_LAUNCH("point_grad_gather", point_grad_gather_kernel, dim3((HW + kThreads - 1) / kThreads, p.B), dim3(kThreads), 0, s, g);
  return launch_status();
}

int launch_gaussian_kl_backward(const float* moments, int B, int n, const float* grad_per_image, float* grad_moments, hipStream_t s) {
  LDMSEG_LAUNCH("gaussian_kl_backward", gaussian_kl_backward_kernel, dim3((2 * n + kThreads - 1) / kThreads, B), dim3(kThreads), 0, s,
                moments, n, grad_per_image, grad_moments);
  return launch_status();
}

}  // namespace ldmseg
