// The seg-VAE's stage-1 loss (trainers_ae.py:204-216), the forward value (its gradient to the logits and the moments is
// point_loss_bwd.hip; what both evaluate per point is point_loss_dev.h): SegmentationLosses.point_loss (losses.py:364-394) - the
// PointRend cross entropy on uncertain points (loss_ce, :303-362) and the per-object BCE + Dice on uncertain points (loss_masks,
// :117-185 with prepare_targets :397-439) - and posterior.kl() (vae.py:416-417).  fp32 NCHW logits x [B,C,H,W], int64 targets
// [B,Ht,Wt], an optional validity mask, and device buffers of uniform draws (nothing is drawn here).
//
//   presence     one launch over the targets: which ids other than ignore_label each image holds once the masked pixels count as
//                ignore_label ([B,C] bytes), and a flag for an id outside [0, C).  The host reads it once: the number of object
//                masks N fixes the shapes of the draws.
//   rows         B cross-entropy rows (one per image) followed by N mask rows (one per object (b, c), by image, then class id).
//   uncertainty  a thread per oversampled point: CE rows sample all C channels bilinearly and keep the top two in registers
//                (second - first, :296-301); mask rows sample their one channel (-|x|, :294).  Only [rows,S] floats are written.
//   select       a workgroup per row: exact top-kU of S by a radix select over the order-preserving bit patterns (four 8-bit LDS
//                histograms), then an index-ordered compaction; ties at the threshold go to the lower index.
//   loss         a thread per point (kU selected + kR fresh): CE rows logsumexp(x / T) - x[label] / T with the nearest-tap label;
//                mask rows BCE-with-logits and the Dice sums against the bilinear sample of (target == c).  fp64 partials per
//                workgroup.
//   finish       one workgroup adds the partials in a fixed order -> {ce, bce, dice}.
//
// Lanes run over POINTS, the channel loop is inside the thread.  A point's four taps sit in one channel plane and the planes are
// H * W * 4 bytes apart, so lanes over channels would touch 64 cache lines to use 4 bytes of each and would need a cross-lane
// top-two; with lanes over points a wave's loads of one channel fall into one plane, neighbouring points share lines, every wave
// of an image walks the planes in the same order (the plane stays in L2 while the image's waves pass), and the top two and the
// running logsumexp never leave registers.
// No float atomics: every float sum is a store of partials plus a fixed-order pass.  Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/ldmseg_hip.h"
#include "../../include/ldmseg_hip_ops.h"
#include "common.h"
#include "kernels.h"
#include "point_loss_dev.h"
#include "point_sample.h"

namespace ldmseg {
namespace {

using namespace pointloss;      // point_loss_dev.h: what the backward (point_loss_bwd.hip) evaluates per point too

// ---------------------------------------------------------------- class presence
__global__ __launch_bounds__(kThreads) void class_presence_kernel(const int64_t* tgt, const uint8_t* valid, int n, int C, int64_t ignore,
                                                                  uint8_t* present, int32_t* flag) {
  __shared__ int s_seen[256];
  const int b = blockIdx.y;
  for (int i = threadIdx.x; i < 256; i += kThreads) s_seen[i] = 0;
  __syncthreads();
  bool bad = false;
  const size_t base = (size_t)b * n;
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
    int64_t v = tgt[base + i];
    if (valid && !valid[base + i]) v = ignore;
    if (v == ignore) continue;
    if (v < 0 || v >= C) { bad = true; continue; }
    if (!s_seen[(int)v]) s_seen[(int)v] = 1;         // (every writer stores the same value)
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += kThreads)
    if (s_seen[c]) present[(size_t)b * C + c] = 1;   // (the table is zeroed by the launcher; workgroups of an image store the same 1)
  if (bad) atomicOr(flag, 1);
}

// ---------------------------------------------------------------- uncertainty
__global__ __launch_bounds__(kThreads) void point_uncertainty_kernel(const PointLoss p) {
#pragma clang fp contract(off)
  const int r = blockIdx.y;
  const int j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= p.S) return;
  const Row w = row_of(p, r);
  const BilinearTaps t = bilinear_taps(w.over[2 * j], w.over[2 * j + 1], p.H, p.W);
  const size_t plane = (size_t)p.H * p.W;
  float u;
  if (w.c < 0) {
    const float* xb = p.x + (size_t)w.b * p.C * plane;
    float first = -INFINITY, second = -INFINITY;
    for (int c = 0; c < p.C; ++c) {
      const float* xc = xb + (size_t)c * plane;
      const float v = bilinear_sample(t, p.H, p.W, [&](int i) { return xc[i]; });
      if (v > first) { second = first; first = v; }
      else if (v > second) second = v;
    }
    u = p.C > 1 ? second - first : 0.0f;
  } else {
    const float* xc = p.x + ((size_t)w.b * p.C + w.c) * plane;
    u = -fabsf(bilinear_sample(t, p.H, p.W, [&](int i) { return xc[i]; }));
  }
  p.unc[(size_t)r * p.S + j] = u + 0.0f;             // -0.0 -> +0.0: equal values get equal keys
}

// ---------------------------------------------------------------- select (keys: f32_key, reduce_dev.h)
__global__ __launch_bounds__(kThreads) void point_select_kernel(const float* unc, int S, int kU, int32_t* sel) {
  __shared__ uint32_t s_hist[256];
  __shared__ uint32_t s_prefix, s_want;
  __shared__ int s_eq[kThreads], s_sel[kThreads];
  const float* u = unc + (size_t)blockIdx.x * S;
  int32_t* out = sel + (size_t)blockIdx.x * kU;
  uint32_t prefix = 0, want = (uint32_t)kU;
  for (int pass = 0; pass < 4; ++pass) {
    for (int i = threadIdx.x; i < 256; i += kThreads) s_hist[i] = 0;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    const uint32_t high_mask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
    for (int i = threadIdx.x; i < S; i += kThreads) {
      const uint32_t key = f32_key(u[i]);
      if ((key & high_mask) == (prefix & high_mask)) atomicAdd(&s_hist[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t above = 0;
      int bin = 255;
      for (; bin > 0; --bin) {                       // the bin that holds the want-th largest; bin 0 takes what is left
        if (above + s_hist[bin] >= want) break;
        above += s_hist[bin];
      }
      s_prefix = prefix | ((uint32_t)bin << shift);
      s_want = want - above;
    }
    __syncthreads();
    prefix = s_prefix; want = s_want;
  }
  // prefix: the key of the kU-th largest; want: how many of its ties are taken, lowest indices first.  Each thread owns a run of
  // consecutive indices, so the output is in index order.
  const int seg = (S + kThreads - 1) / kThreads;
  const int lo = min(S, (int)threadIdx.x * seg), hi = min(S, lo + seg);
  int gt = 0, eq = 0;
  for (int i = lo; i < hi; ++i) {
    const uint32_t key = f32_key(u[i]);
    gt += key > prefix;
    eq += key == prefix;
  }
  s_eq[threadIdx.x] = eq; s_sel[threadIdx.x] = gt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int eq_run = 0, sel_run = 0;
    for (int t = 0; t < kThreads; ++t) {
      const int e = s_eq[t], g = s_sel[t];
      const int left = (int)want - eq_run;
      const int take = e < left ? e : (left > 0 ? left : 0);
      s_eq[t] = eq_run; s_sel[t] = sel_run;
      eq_run += e; sel_run += g + take;
    }
  }
  __syncthreads();
  int eq_rank = s_eq[threadIdx.x], pos = s_sel[threadIdx.x];
  for (int i = lo; i < hi; ++i) {
    const uint32_t key = f32_key(u[i]);
    bool take = key > prefix;
    if (key == prefix) { take = eq_rank < (int)want; ++eq_rank; }
    if (take && pos < kU) out[pos++] = i;
  }
}

// ---------------------------------------------------------------- loss
// partial[(r * nchunk + chunk) * 4 + k]: CE rows {sum of point losses, kept points, -, -}; mask rows {bce, sigmoid * t, sigmoid, t}
__global__ __launch_bounds__(kThreads) void point_loss_kernel(const PointLoss p) {
#pragma clang fp contract(off)
  __shared__ double s_red[kThreads / 64];
  const int r = blockIdx.y;
  const int j = blockIdx.x * kThreads + threadIdx.x;
  const Row w = row_of(p, r);
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  if (j < p.P) {
    const PointUV u = point_uv(p, w, r, j);
    const BilinearTaps t = bilinear_taps(u.x, u.y, p.H, p.W);
    if (w.c < 0) {
      const CePoint q = ce_point(p, w, u, t);
      if (q.kept) {
        a0 = ((double)q.mx + log(q.sum)) - (double)q.at_label;
        a1 = 1.0;
      }
    } else {
      const MaskPoint q = mask_point(p, w, u, t);
      // binary_cross_entropy_with_logits: (1 - y) * x + max(-x, 0) + log(1 + exp(-|x|))
      const double xd = (double)q.x, yd = (double)q.y;
      a0 = (1.0 - yd) * xd + (xd < 0.0 ? -xd : 0.0) + log1p(exp(-fabs(xd)));
      const double sg = (double)q.sg;
      a1 = sg * yd; a2 = sg; a3 = yd;
    }
  }
  const double t0 = block_sum(a0, s_red), t1 = block_sum(a1, s_red), t2 = block_sum(a2, s_red), t3 = block_sum(a3, s_red);
  if (threadIdx.x == 0) {
    double* q = p.partial + ((size_t)r * gridDim.x + blockIdx.x) * 4;
    q[0] = t0; q[1] = t1; q[2] = t2; q[3] = t3;
  }
}

// out[0] = ce, out[1] = sum of the mask rows' BCE / num_masks, out[2] = sum of their Dice losses / num_masks
__global__ __launch_bounds__(kThreads) void point_loss_finish_kernel(const double* partial, int B, int N, int nchunk, int P, double num_masks,
                                                                     float* out) {
  __shared__ double s_red[kThreads / 64];
  double ce = 0.0, cnt = 0.0;
  for (int i = threadIdx.x; i < B * nchunk; i += kThreads) { ce += partial[(size_t)i * 4]; cnt += partial[(size_t)i * 4 + 1]; }
  const double ce_t = block_sum(ce, s_red), cnt_t = block_sum(cnt, s_red);
  double bce = 0.0, dice = 0.0;
  for (int m = threadIdx.x; m < N; m += kThreads) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    const double* q = partial + (size_t)(B + m) * nchunk * 4;
    for (int c = 0; c < nchunk; ++c) { a0 += q[4 * c]; a1 += q[4 * c + 1]; a2 += q[4 * c + 2]; a3 += q[4 * c + 3]; }
    bce += a0 / (double)P;
    dice += 1.0 - (2.0 * a1 + 1.0) / (a2 + a3 + 1.0);
  }
  const double bce_t = block_sum(bce, s_red), dice_t = block_sum(dice, s_red);
  if (threadIdx.x == 0) {
    out[0] = (float)(ce_t / cnt_t);                  // no kept point: 0 / 0 = NaN, like F.cross_entropy
    out[1] = N > 0 ? (float)(bce_t / num_masks) : 0.0f;
    out[2] = N > 0 ? (float)(dice_t / num_masks) : 0.0f;
  }
}

// ---------------------------------------------------------------- KL
// a workgroup per image: 0.5 * sum(mean^2 + exp(logvar) - 1 - logvar), logvar clamped to [-30, 20] (vae.py:389, :417)
__global__ __launch_bounds__(kThreads) void gaussian_kl_kernel(const float* moments, int n, float* per_image) {
  __shared__ double s_red[kThreads / 64];
  const float* mean = moments + (size_t)blockIdx.x * 2 * n;
  const float* logvar = mean + n;
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += kThreads) {
    const float m = mean[i];
    const float lv = fminf(fmaxf(logvar[i], -30.0f), 20.0f);
    acc += (double)(((m * m + expf(lv)) - 1.0f) - lv);
  }
  const double t = block_sum(acc, s_red);
  if (threadIdx.x == 0) per_image[blockIdx.x] = (float)(0.5 * t);
}

__global__ __launch_bounds__(64) void gaussian_kl_finish_kernel(const float* per_image, int B, float* mean) {
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int b = 0; b < B; ++b) t += (double)per_image[b];
    mean[0] = (float)(t / (double)B);
  }
}


// scratch layout of launch_point_loss (bytes): partials | uncertainties | selected indices
struct PointScratch {
  size_t partial, unc, sel, total;
};
inline PointScratch point_scratch(int rows, int S, int kU, int P) {
  PointScratch l;
  const size_t nchunk = (size_t)(P + kThreads - 1) / kThreads;
  l.partial = 0;
  l.unc = up16(l.partial + (size_t)rows * nchunk * 4 * sizeof(double));
  l.sel = up16(l.unc + (size_t)rows * S * sizeof(float));
  l.total = up16(l.sel + (size_t)rows * kU * sizeof(int32_t));
  return l;
}

}  // namespace

int launch_class_presence(const int64_t* targets, const uint8_t* valid, int B, int Ht, int Wt, int C, int64_t ignore_label,
                          uint8_t* present, int32_t* flag, hipStream_t s) {
  const int n = Ht * Wt;                             // (arguments are checked by ldmseg_class_presence, the one caller)
  if (hipMemsetAsync(present, 0, (size_t)B * C, s) != hipSuccess) return -3;
  if (hipMemsetAsync(flag, 0, sizeof(int32_t), s) != hipSuccess) return -3;
  int gx = (n + kThreads * 16 - 1) / (kThreads * 16);
  gx = gx < 1 ? 1 : (gx > 64 ? 64 : gx);
  LDMSEG_LAUNCH("class_presence", class_presence_kernel, dim3(gx, B), dim3(kThreads), 0, s, targets, valid, n, C, ignore_label, present,
                flag);
  return launch_status();
}

size_t point_loss_scratch_bytes(int rows, int S, int kU, int P) {
  if (rows < 1 || S < 0 || kU < 0 || P < 1) return 0;
  return point_scratch(rows, S, kU, P).total;
}

int launch_point_loss(const PointLoss& in, double num_masks, float* out, int32_t* selected, void* scratch, hipStream_t s) {
  PointLoss p = in;                                  // (arguments are checked by ldmseg_point_loss, the one caller)
  const int rows = p.B + p.N;
  const PointScratch l = point_scratch(rows, p.S, p.kU, p.P);
  char* sc = (char*)scratch;
  p.partial = (double*)(sc + l.partial);
  p.unc = (float*)(sc + l.unc);
  p.sel = selected ? selected : (int32_t*)(sc + l.sel);
  const int nchunk = (p.P + kThreads - 1) / kThreads;
  if (p.kU > 0) {
    LDMSEG_LAUNCH("point_uncertainty", point_uncertainty_kernel, dim3((p.S + kThreads - 1) / kThreads, rows), dim3(kThreads), 0, s, p);
    LDMSEG_LAUNCH("point_select", point_select_kernel, dim3(rows), dim3(kThreads), 0, s, (const float*)p.unc, p.S, p.kU, p.sel);
  }
  LDMSEG_LAUNCH("point_loss", point_loss_kernel, dim3(nchunk, rows), dim3(kThreads), 0, s, p);
  LDMSEG_LAUNCH("point_loss_finish", point_loss_finish_kernel, dim3(1), dim3(kThreads), 0, s, (const double*)p.partial, p.B, p.N, nchunk,
                p.P, num_masks, out);
  return launch_status();
}

int launch_gaussian_kl(const float* moments, int B, int n, float* per_image, float* mean, hipStream_t s) {
  LDMSEG_LAUNCH("gaussian_kl", gaussian_kl_kernel, dim3(B), dim3(kThreads), 0, s, moments, n, per_image);
  if (mean) LDMSEG_LAUNCH("gaussian_kl_finish", gaussian_kl_finish_kernel, dim3(1), dim3(64), 0, s, (const float*)per_image, B, mean);
  return launch_status();
}

}  // namespace ldmseg

using namespace ldmseg;

extern "C" {

// the tap rule of point_sample.h, evaluated on the host: CPU-suite test hook
int ldmseg_op_point_taps(int n, const float* u, int H, int W, int mode, int32_t* index, float* weight) {
  if (n < 0 || !u || !index || H < 1 || W < 1 || (mode != 0 && mode != 1) || (mode == 0 && !weight)) return LDMSEG_E_ARG;
  for (int i = 0; i < n; ++i) {
    if (mode == 1) { index[i] = nearest_tap(u[2 * i], u[2 * i + 1], H, W); continue; }
    const BilinearTaps t = bilinear_taps(u[2 * i], u[2 * i + 1], H, W);
    const float w4[4] = {t.nw, t.ne, t.sw, t.se};
    for (int k = 0; k < 4; ++k) {
      const int x = t.x0 + (k & 1), y = t.y0 + (k >> 1);
      index[4 * i + k] = tap_inside(x, y, H, W) ? y * W + x : -1;
      weight[4 * i + k] = w4[k];
    }
  }
  return 0;
}

}
