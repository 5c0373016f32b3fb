// The forward half of the training step behind the UNet output (trainers_ldm_cond.py:495-661), fp32, memory bound:
//
//   loss tail    one launch over prediction / target / noisy [B,C,HW]: the element loss of loss_fn (:515-525) times the
//                scheduler weight of the sample's timestep (:597), pred_latents (:605-615, clamp of :492), and one fp64 partial
//                sum per workgroup; a one-workgroup finish adds the partials in a fixed order -> per-sample sums and the mean.
//   OHEM         torch.topk(loss, k)[0].mean() (:600-602) as a radix select over the order-preserving bit patterns of the
//                element losses: four 8-bit histogram passes (LDS histogram per workgroup, integer atomics to the global one)
//                find the k-th largest value, one pass sums what is strictly larger; ties enter as count * value.
//   mask         get_loss_weight_mask (:643-661): nearest resize (nearest_index.h) + ignore / padding / 1 / count(id) per image.
//   min / max    of a tensor into a device {min, max} pair (predict_sample's clamp bounds, :492).
//
// No float atomics: every float sum is a store of partials plus a fixed-order pass, so two runs agree bit for bit.  Compiled with
// -ffp-contract=off: each product / difference of the element loss is rounded separately, like the reference's torch ops.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/ldmseg_hip.h"
#include "common.h"
#include "kernels.h"
#include "nearest_index.h"
#include "reduce_dev.h"
#include "sched_math.h"

namespace ldmseg {
namespace {

constexpr int kThreads = 256;
constexpr int kPerThread = 4;
constexpr int kChunk = kThreads * kPerThread;     // elements of one sample per workgroup of the loss tail
constexpr int kMaxBlocks = 256;                   // grid cap of the grid-stride passes (OHEM, min / max)

static_assert(kThreads == kBlockSumThreads, "block_sum (reduce_dev.h) sums kBlockSumThreads / 64 waves");

// ---------------------------------------------------------------- loss tail
__device__ __forceinline__ float elem_loss(float x, float y, int loss_type) {
#pragma clang fp contract(off)
  const float d = __fsub_rn(x, y);
  if (loss_type == LDMSEG_LOSS_L1) return fabsf(d);
  if (loss_type == LDMSEG_LOSS_L2) return __fmul_rn(d, d);
  const float z = fabsf(d);                        // smooth_l1, beta = 1: z < 1 ? 0.5 * z * z : z - 0.5
  return z < 1.0f ? __fmul_rn(__fmul_rn(0.5f, z), z) : __fsub_rn(z, 0.5f);
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void loss_tail_kernel(const LossTail p) {
#pragma clang fp contract(off)
  __shared__ double s_red[kThreads / 64];
  const int b = blockIdx.y;
  const size_t base = (size_t)b * p.per;
  const int64_t tb = clamp_timestep(p.t[b], p.n_train);
  const NoiseCoef nc = noise_coef(p.ac[tb], 1.0f);
  const float wt = p.weights ? p.weights[tb] : 1.0f;
  float lo = 0.f, hi = 0.f;
  if (p.minmax) { lo = p.minmax[0]; hi = p.minmax[1]; }

  int e[kPerThread];
  float x[kPerThread], y[kPerThread], z[kPerThread], src[kPerThread];
  uint8_t pm[kPerThread];
  const bool need_noisy = p.pred_latents && p.pred_type == 0;
  if (VEC) {                                       // per % 4 == 0 and 16-byte aligned bases: a thread's four are all in or all out
    const int e0 = blockIdx.x * kChunk + threadIdx.x * kPerThread;
    const bool in = e0 < p.per;
    float4 vx = {0, 0, 0, 0}, vy = vx, vz = vx, vs = vx;
    uchar4 vm = {0, 0, 0, 0};
    if (in) {
      vx = *reinterpret_cast<const float4*>(p.pred + base + e0);
      if (p.target) vy = *reinterpret_cast<const float4*>(p.target + base + e0);
      if (need_noisy) vz = *reinterpret_cast<const float4*>(p.noisy + base + e0);
      if (p.paste) {
        vm = *reinterpret_cast<const uchar4*>(p.paste + base + e0);
        vs = *reinterpret_cast<const float4*>(p.paste_src + base + e0);
      }
    }
    x[0] = vx.x; x[1] = vx.y; x[2] = vx.z; x[3] = vx.w;
    y[0] = vy.x; y[1] = vy.y; y[2] = vy.z; y[3] = vy.w;
    z[0] = vz.x; z[1] = vz.y; z[2] = vz.z; z[3] = vz.w;
    src[0] = vs.x; src[1] = vs.y; src[2] = vs.z; src[3] = vs.w;
    pm[0] = vm.x; pm[1] = vm.y; pm[2] = vm.z; pm[3] = vm.w;
    for (int j = 0; j < kPerThread; ++j) e[j] = in ? e0 + j : -1;
  } else {
    for (int j = 0; j < kPerThread; ++j) {
      const int ej = blockIdx.x * kChunk + j * kThreads + threadIdx.x;
      const bool in = ej < p.per;
      e[j] = in ? ej : -1;
      x[j] = in ? p.pred[base + ej] : 0.f;
      y[j] = (in && p.target) ? p.target[base + ej] : 0.f;
      z[j] = (in && need_noisy) ? p.noisy[base + ej] : 0.f;
      pm[j] = (in && p.paste) ? p.paste[base + ej] : (uint8_t)0;
      src[j] = (in && p.paste && pm[j]) ? p.paste_src[base + ej] : 0.f;
    }
  }

  double acc = 0.0;
  float lv[kPerThread], pv[kPerThread];
  for (int j = 0; j < kPerThread; ++j) {
    lv[j] = 0.f; pv[j] = 0.f;
    if (e[j] < 0) continue;
    if (p.target) {
      float l = elem_loss(x[j], y[j], p.loss_type);
      if (p.mask) l = __fmul_rn(l, p.mask[(size_t)b * p.HW + (e[j] % p.HW)]);
      if (p.weights) l = __fmul_rn(l, wt);
      lv[j] = l;
      acc += (double)l;
    }
    if (p.pred_latents) {
      float v = p.pred_type == 0 ? remove_noise_elem(z[j], x[j], nc) : x[j];
      if (pm[j]) v = src[j];
      if (p.minmax) {                              // torch.clamp(v, lo, hi) = min(max(v, lo), hi): a NaN in v, lo or hi comes out
        v = (lo != lo) ? lo : (v < lo ? lo : v);   // (latents with a NaN make ldmseg_tensor_minmax write a NaN pair)
        v = (hi != hi) ? hi : (v > hi ? hi : v);
      }
      pv[j] = v;
    }
  }
  if (VEC) {
    if (e[0] >= 0) {
      if (p.elem && p.target) *reinterpret_cast<float4*>(p.elem + base + e[0]) = make_float4(lv[0], lv[1], lv[2], lv[3]);
      if (p.pred_latents) *reinterpret_cast<float4*>(p.pred_latents + base + e[0]) = make_float4(pv[0], pv[1], pv[2], pv[3]);
    }
  } else {
    for (int j = 0; j < kPerThread; ++j) {
      if (e[j] < 0) continue;
      if (p.elem && p.target) p.elem[base + e[j]] = lv[j];
      if (p.pred_latents) p.pred_latents[base + e[j]] = pv[j];
    }
  }
  const double t = block_sum(acc, s_red);
  if (threadIdx.x == 0) p.partial[(size_t)b * gridDim.x + blockIdx.x] = t;
}

// ---------------------------------------------------------------- OHEM: radix select (keys: f32_key / key_f32, reduce_dev.h)
struct SelectState {     // after `pass` digits: the key prefix of the k-th largest and how many of that prefix are still wanted
  uint32_t prefix;
  uint32_t pad;
  uint64_t want;
};

// state[pass] from state[pass - 1] and the histogram of digit pass - 1 (every workgroup derives it for itself; workgroup 0 also
// stores it for the next launch).  pass in 1..4.
__device__ __forceinline__ SelectState select_derive(const uint32_t* hist, const SelectState* state, int pass, uint64_t k,
                                                     uint32_t* s_hist, SelectState* s_state) {
  const uint32_t* h = hist + (size_t)(pass - 1) * 256;
  for (int i = threadIdx.x; i < 256; i += kThreads) s_hist[i] = h[i];
  __syncthreads();
  if (threadIdx.x == 0) {
    SelectState prev;
    if (pass == 1) { prev.prefix = 0; prev.pad = 0; prev.want = k; }
    else prev = state[pass - 1];
    const int shift = 24 - 8 * (pass - 1);
    uint64_t above = 0;
    int bin = 255;
    for (; bin > 0; --bin) {                       // the bin that holds the want-th largest; bin 0 takes what is left
      if (above + s_hist[bin] >= prev.want) break;
      above += s_hist[bin];
    }
    SelectState st;
    st.prefix = prev.prefix | ((uint32_t)bin << shift);
    st.pad = 0;
    st.want = prev.want - above;
    *s_state = st;
  }
  __syncthreads();
  return *s_state;
}

__global__ __launch_bounds__(kThreads) void ohem_hist_kernel(const float* elem, size_t n, int pass, uint64_t k, uint32_t* hist,
                                                             SelectState* state) {
  __shared__ uint32_t s_hist[256];
  __shared__ uint32_t s_prev[256];
  __shared__ SelectState s_state;
  uint32_t prefix = 0;
  if (pass > 0) {
    const SelectState st = select_derive(hist, state, pass, k, s_prev, &s_state);
    if (blockIdx.x == 0 && threadIdx.x == 0) state[pass] = st;
    prefix = st.prefix;
  }
  for (int i = threadIdx.x; i < 256; i += kThreads) s_hist[i] = 0;
  __syncthreads();
  const int shift = 24 - 8 * pass;
  const uint32_t high_mask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) {
    const uint32_t key = f32_key(elem[i]);
    if ((key & high_mask) == (prefix & high_mask)) atomicAdd(&s_hist[(key >> shift) & 255u], 1u);
  }
  __syncthreads();
  uint32_t* h = hist + (size_t)pass * 256;
  for (int i = threadIdx.x; i < 256; i += kThreads)
    if (s_hist[i]) atomicAdd(&h[i], s_hist[i]);
}

// fp64 sum of the elements strictly above the k-th largest (a NaN element is added whatever its key: topk ranks NaN first)
__global__ __launch_bounds__(kThreads) void ohem_sum_kernel(const float* elem, size_t n, uint64_t k, const uint32_t* hist,
                                                            SelectState* state, double* partial) {
  __shared__ uint32_t s_prev[256];
  __shared__ SelectState s_state;
  __shared__ double s_red[kThreads / 64];
  const SelectState st = select_derive(hist, state, 4, k, s_prev, &s_state);
  if (blockIdx.x == 0 && threadIdx.x == 0) state[4] = st;
  double acc = 0.0;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) {
    const float v = elem[i];
    if (v != v || f32_key(v) > st.prefix) acc += (double)v;
  }
  const double t = block_sum(acc, s_red);
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// ---------------------------------------------------------------- finish: per-sample sums, mean
__global__ __launch_bounds__(kThreads) void loss_finish_kernel(const double* partial, int B, int nchunk, double count,
                                                               float* sample_sums, float* mean, const double* ohem_partial,
                                                               int ohem_blocks, const SelectState* state, double k) {
  __shared__ double s_total[kThreads / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // a wave per sample: lanes stride over the sample's partials, xor tree; the waves' samples are added in sample order below
  double wave_total = 0.0;
  for (int b = wave; b < B; b += kThreads / 64) {
    double v = 0.0;
    for (int c = lane; c < nchunk; c += 64) v += partial[(size_t)b * nchunk + c];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0 && sample_sums) sample_sums[b] = (float)v;
    wave_total += v;
  }
  double ohem = 0.0;
  if (ohem_partial && wave == 0) {
    for (int c = lane; c < ohem_blocks; c += 64) ohem += ohem_partial[c];
    for (int o = 32; o > 0; o >>= 1) ohem += __shfl_xor(ohem, o);
  }
  if (lane == 0) s_total[wave] = wave_total;
  __syncthreads();
  if (threadIdx.x == 0) {
    if (ohem_partial) {
      const SelectState st = state[4];
      mean[0] = (float)((ohem + (double)st.want * (double)key_f32(st.prefix)) / k);
    } else {
      double t = 0.0;
      for (int w = 0; w < kThreads / 64; ++w) t += s_total[w];
      mean[0] = (float)(t / count);
    }
  }
}

// ---------------------------------------------------------------- min / max
__global__ __launch_bounds__(kThreads) void minmax_kernel(const float* x, size_t n, float* partial) {
  __shared__ float s_lo[kThreads / 64], s_hi[kThreads / 64];
  __shared__ int s_nan[kThreads / 64];
  float lo = INFINITY, hi = -INFINITY;
  int nan = 0;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) {
    const float v = x[i];
    if (v != v) nan = 1;
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
  }
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, o));
    hi = fmaxf(hi, __shfl_xor(hi, o));
    nan |= __shfl_xor(nan, o);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { s_lo[wave] = lo; s_hi[wave] = hi; s_nan[wave] = nan; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kThreads / 64; ++w) { lo = fminf(lo, s_lo[w]); hi = fmaxf(hi, s_hi[w]); nan |= s_nan[w]; }
    partial[3 * blockIdx.x + 0] = lo;
    partial[3 * blockIdx.x + 1] = hi;
    partial[3 * blockIdx.x + 2] = nan ? 1.f : 0.f;
  }
}

__global__ __launch_bounds__(64) void minmax_finish_kernel(const float* partial, int blocks, float* out) {
  float lo = INFINITY, hi = -INFINITY, nan = 0.f;
  for (int c = threadIdx.x; c < blocks; c += 64) {
    lo = fminf(lo, partial[3 * c]);
    hi = fmaxf(hi, partial[3 * c + 1]);
    nan = fmaxf(nan, partial[3 * c + 2]);
  }
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, o));
    hi = fmaxf(hi, __shfl_xor(hi, o));
    nan = fmaxf(nan, __shfl_xor(nan, o));
  }
  if (threadIdx.x == 0) {                          // tensor.min() / .max() of a tensor with a NaN is NaN
    out[0] = nan > 0.f ? NAN : lo;
    out[1] = nan > 0.f ? NAN : hi;
  }
}

// ---------------------------------------------------------------- loss-weight mask
struct MaskParams {
  const void* src;       // [B][Hi][Wi]
  int src_dtype;         // 0 int64, 1 uint8 / bool, 2 fp32
  int Hi, Wi, h, w;
  float scale_h, scale_w;
  int mode;              // LDMSEG_MASK_*
  float ignore;          // float(ignore_label): the reference compares the resized fp32 map
  float* out;            // [B][h][w]
  int32_t* flag;
};

__device__ __forceinline__ float mask_src(const MaskParams& p, size_t i) {
  if (p.src_dtype == 0) return (float)((const int64_t*)p.src)[i];
  if (p.src_dtype == 1) return (float)((const uint8_t*)p.src)[i];
  return ((const float*)p.src)[i];
}

// one workgroup per image
__global__ __launch_bounds__(kThreads) void loss_mask_kernel(const MaskParams p) {
#pragma clang fp contract(off)
  __shared__ int s_cnt[256];
  const int b = blockIdx.x;
  const size_t in_base = (size_t)b * p.Hi * p.Wi;
  const int n = p.h * p.w;
  float* out = p.out + (size_t)b * n;
  if (p.mode == LDMSEG_MASK_COUNTS) {
    for (int i = threadIdx.x; i < 256; i += kThreads) s_cnt[i] = 0;
    __syncthreads();
  }
  bool bad = false;
  for (int pass = (p.mode == LDMSEG_MASK_COUNTS ? 0 : 1); pass < 2; ++pass) {
    for (int i = threadIdx.x; i < n; i += kThreads) {
      const int oy = i / p.w, ox = i - oy * p.w;
      const int sy = nearest_src_index_scaled(oy, p.scale_h, p.Hi), sx = nearest_src_index_scaled(ox, p.scale_w, p.Wi);
      const float v = mask_src(p, in_base + (size_t)sy * p.Wi + sx);
      if (p.mode == LDMSEG_MASK_IGNORE) { out[i] = v != p.ignore ? 1.0f : 0.0f; continue; }
      if (p.mode == LDMSEG_MASK_PADDING) { out[i] = v; continue; }
      if (v == p.ignore) { if (pass) out[i] = 0.0f; continue; }
      const int id = (v >= 0.0f && v < 256.0f) ? (int)v : -1;
      if (id < 0 || (float)id != v) {              // outside the table (or not an integer): flagged, and a NaN weight shows in the loss
        bad = true;
        if (pass) out[i] = NAN;
        continue;
      }
      if (pass == 0) atomicAdd(&s_cnt[id], 1);
      else out[i] = __fdiv_rn(1.0f, (float)s_cnt[id]);
    }
    __syncthreads();
  }
  if (bad) atomicOr(p.flag, 1);
}

inline bool aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
inline int stride_blocks(size_t n) {
  const size_t g = (n + kChunk - 1) / kChunk;
  return (int)(g < 1 ? 1 : (g > (size_t)kMaxBlocks ? kMaxBlocks : g));
}

// scratch layout of launch_diffusion_loss (bytes): partials | ohem partials | select states | histograms
struct LossScratch {
  size_t partial, ohem_partial, state, hist, total;
};
inline LossScratch loss_scratch(int B, int nchunk) {
  LossScratch l;
  l.partial = 0;
  l.ohem_partial = l.partial + (size_t)B * nchunk * sizeof(double);
  l.state = l.ohem_partial + (size_t)kMaxBlocks * sizeof(double);
  l.hist = l.state + 5 * sizeof(SelectState);
  l.total = l.hist + 4 * 256 * sizeof(uint32_t);
  return l;
}

}  // namespace

size_t diffusion_loss_scratch_bytes(int B, int C, int HW) {
  if (B < 1 || C < 1 || HW < 1) return 0;
  const size_t per = (size_t)C * HW;
  return loss_scratch(B, (int)((per + kChunk - 1) / kChunk)).total;
}

int launch_diffusion_loss(const LossTail& in, int B, double ohem_k, float* sample_sums, float* mean, void* scratch, hipStream_t s) {
  LossTail p = in;                                 // (arguments are checked by ldmseg_diffusion_loss, the one caller)
  p.per = p.C * p.HW;
  const int nchunk = (p.per + kChunk - 1) / kChunk;
  const LossScratch l = loss_scratch(B, nchunk);
  char* sc = (char*)scratch;
  p.partial = (double*)(sc + l.partial);
  const bool ohem = ohem_k > 0 && p.target;
  const bool vec = p.per % 4 == 0 && aligned(p.pred, 16) && aligned(p.target, 16) && aligned(p.noisy, 16) && aligned(p.paste, 4) &&
                   aligned(p.paste_src, 16) && aligned(p.elem, 16) && aligned(p.pred_latents, 16);
  if (ohem && hipMemsetAsync(sc + l.hist, 0, 4 * 256 * sizeof(uint32_t), s) != hipSuccess) return -3;
  if (vec) LDMSEG_LAUNCH(launch_name("loss_tail<vec,loss=%d,pred=%d>", p.loss_type, p.pred_type), loss_tail_kernel<true>,
                         dim3(nchunk, B), dim3(kThreads), 0, s, p);
  else LDMSEG_LAUNCH(launch_name("loss_tail<scalar,loss=%d,pred=%d>", p.loss_type, p.pred_type), loss_tail_kernel<false>,
                     dim3(nchunk, B), dim3(kThreads), 0, s, p);
  if (!p.target) return launch_status();                      // pred_latents only: no loss, so nothing to finish (mean / sample_sums may be null)
  const size_t n = (size_t)B * p.per;
  int oblocks = 0;
  if (ohem) {
    oblocks = stride_blocks(n);
    uint32_t* hist = (uint32_t*)(sc + l.hist);
    SelectState* state = (SelectState*)(sc + l.state);
    for (int pass = 0; pass < 4; ++pass)
      LDMSEG_LAUNCH(launch_name("ohem_hist<pass=%d>", pass), ohem_hist_kernel, dim3(oblocks), dim3(kThreads), 0, s, p.elem, n, pass,
                    (uint64_t)ohem_k, hist, state);
    LDMSEG_LAUNCH("ohem_sum", ohem_sum_kernel, dim3(oblocks), dim3(kThreads), 0, s, p.elem, n, (uint64_t)ohem_k, hist, state,
                  (double*)(sc + l.ohem_partial));
  }
  LDMSEG_LAUNCH("loss_finish", loss_finish_kernel, dim3(1), dim3(kThreads), 0, s, p.partial, B, nchunk, (double)n, sample_sums, mean,
                ohem ? (const double*)(sc + l.ohem_partial) : (const double*)nullptr, oblocks,
                (const SelectState*)(sc + l.state), ohem_k);
  return launch_status();
}

size_t tensor_minmax_scratch_bytes() { return (size_t)kMaxBlocks * 3 * sizeof(float); }

int launch_tensor_minmax(const float* x, size_t n, float* out, void* scratch, hipStream_t s) {
  const int blocks = stride_blocks(n);
  LDMSEG_LAUNCH("tensor_minmax", minmax_kernel, dim3(blocks), dim3(kThreads), 0, s, x, n, (float*)scratch);
  LDMSEG_LAUNCH("tensor_minmax_finish", minmax_finish_kernel, dim3(1), dim3(64), 0, s, (const float*)scratch, blocks, out);
  return launch_status();
}

int launch_loss_weight_mask(const void* src, int src_dtype, int B, int Hi, int Wi, int h, int w, int mode, int64_t ignore_label,
                            float* out, int32_t* flag, hipStream_t s) {
  MaskParams p;                                    // (arguments are checked by ldmseg_loss_weight_mask, the one caller)
  p.src = src; p.src_dtype = src_dtype;
  p.Hi = Hi; p.Wi = Wi; p.h = h; p.w = w;
  p.scale_h = nearest_scale(Hi, h);                // on the host: one IEEE fp32 division, like torch's
  p.scale_w = nearest_scale(Wi, w);
  p.mode = mode;
  p.ignore = (float)ignore_label;
  p.out = out; p.flag = flag;
  if (hipMemsetAsync(flag, 0, sizeof(int32_t), s) != hipSuccess) return -3;
  LDMSEG_LAUNCH(launch_name("loss_mask<mode=%d,src=%d>", mode, src_dtype), loss_mask_kernel, dim3(B), dim3(kThreads), 0, s, p);
  return launch_status();
}

}  // namespace ldmseg
