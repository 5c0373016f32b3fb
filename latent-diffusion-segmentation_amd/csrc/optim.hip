// The weight update of the training step (the reference's optim.py + trainers_ae.py:305-325: clip_grad_norm_(..., 3.0) and
// torch.optim.AdamW) over a LIST of fp32 tensors, memory bound, and its three C entries (ldmseg_grad_norm / _grad_clip / _adamw_step).
//
//   norm pass    a workgroup owns one chunk (kChunk elements) of one tensor at a time: squares and adds it in fp64 (block_sum,
//                reduce_dev.h) and stores ONE partial per chunk.
//   finish       one workgroup adds the partials (only for lists of more than one launch, more than kInlinePartials chunks, or
//                when the norm is all that is asked for) -> one fp64 sum, and the norm as a float.
//   update pass  every workgroup adds the partials for itself, all in the same fixed order (so all get the same bits), makes
//                coef = min(1, max_norm / (norm + 1e-6)) in fp32, then walks its chunks: g *= coef (stored back), AdamW.
//
// Pointers and the per-tensor scalars travel in the kernel arguments (MultiLaunch, below 4 KiB): no table is copied to the device,
// nothing is read back, everything is ordered by the stream.  The chunk table is the prefix `chunk0` of each tensor's first chunk,
// built on the host from the numels; grids are capped at kMaxGrid and loop over chunks.  No float atomics: two calls agree bit for
// bit.  Compiled with -ffp-contract=off: every product, sum and quotient of the update is rounded separately, in torch's order.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "reduce_dev.h"
#include "runtime.h"

namespace ldmseg {
namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 8192;                       // elements of one tensor per workgroup and loop step: 32 per thread
constexpr int kMaxTensors = LDMSEG_MULTI_TENSOR_PER_LAUNCH;
constexpr int kMaxChunks = 1 << 18;                // chunks of one launch (2^31 elements); a tensor with more is cut into runs of whole chunks
constexpr int kMaxGrid = 2048;                     // 256 CUs x 8 workgroups
constexpr int kInlinePartials = 2048;              // up to here the update pass adds the partials itself (no finish launch)

static_assert(kThreads == kBlockSumThreads, "block_sum (reduce_dev.h) sums kBlockSumThreads / 64 waves");
static_assert(kChunk % 4 == 0, "a chunk boundary keeps the tensor's 16-byte phase");

enum { MODE_CLIP = 0, MODE_ADAMW = 1, MODE_CLIP_ADAMW = 2 };

struct Seg {                                       // one tensor, or a run of whole chunks of a very long one
  float* p; float* g; float* m; float* v;
  int64_t numel;
  float decay, omb1, b2, omb2, step_size, bc2_sqrt, eps;   // 1 - lr wd | 1 - beta1 | beta2 | 1 - beta2 | lr / bc1 | sqrt(bc2) | eps
  int chunk0;                                      // the segment's first chunk within the launch
};

struct MultiLaunch {
  Seg seg[kMaxTensors];
  int nseg, nchunks;
  int64_t partial0;                                // norm pass: index of the launch's first chunk among the call's partials
  double* partials;                                // norm pass: out; update pass: what to add (npartials of them)
  int npartials;
  float max_norm;
  float* total_out;                                // update pass: workgroup 0 stores the norm here (NULL: the finish launch did)
};
static_assert(sizeof(MultiLaunch) <= 4096, "the launch description travels as kernel arguments");

__device__ __forceinline__ uintptr_t addr(const void* p) { return (uintptr_t)p; }

// elements in front of the first 16-byte boundary of a chunk that starts at g (all of it when `same` is false: scalar chunk)
__device__ __forceinline__ int head_of(const float* g, int len, bool same) {
  const int h = (int)(((16 - (addr(g) & 15)) & 15) >> 2);
  return (same && h < len) ? h : len;
}

// sum of n partials in one fixed order (thread t adds t, t + 256, ...; then block_sum): the same bits in every workgroup.  In thread 0.
__device__ __forceinline__ double sum_partials(const double* partials, int n, double* s_red) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += kThreads) acc += partials[i];
  return block_sum(acc, s_red);
}

__device__ __forceinline__ int seg_of(const MultiLaunch& a, int c, int i) {
  while (i + 1 < a.nseg && a.seg[i + 1].chunk0 <= c) ++i;
  return i;
}

__global__ __launch_bounds__(kThreads) void grad_sumsq_kernel(const MultiLaunch a) {
  __shared__ double s_red[kThreads / 64];
  int i = 0;
  for (int c = blockIdx.x; c < a.nchunks; c += gridDim.x) {
    i = seg_of(a, c, i);
    const int64_t off = (int64_t)(c - a.seg[i].chunk0) * kChunk;
    const int64_t left = a.seg[i].numel - off;
    const int len = left < kChunk ? (int)left : kChunk;
    const float* g = a.seg[i].g + off;
    const int head = head_of(g, len, true);
    const int nvec = (len - head) >> 2;
    double acc = 0.0;
    for (int e = threadIdx.x; e < head; e += kThreads) acc += (double)g[e] * (double)g[e];
    for (int k = threadIdx.x; k < nvec; k += kThreads) {
      const float4 x = *reinterpret_cast<const float4*>(g + head + 4 * k);
      acc += (double)x.x * (double)x.x;
      acc += (double)x.y * (double)x.y;
      acc += (double)x.z * (double)x.z;
      acc += (double)x.w * (double)x.w;
    }
    for (int e = head + 4 * nvec + threadIdx.x; e < len; e += kThreads) acc += (double)g[e] * (double)g[e];
    const double t = block_sum(acc, s_red);
    if (threadIdx.x == 0) a.partials[a.partial0 + c] = t;
  }
}

__global__ __launch_bounds__(kThreads) void grad_norm_finish_kernel(const double* partials, int n, double* sum, float* total_out) {
  __shared__ double s_red[kThreads / 64];
  const double t = sum_partials(partials, n, s_red);
  if (threadIdx.x == 0) {
    sum[0] = t;
    if (total_out) total_out[0] = (float)sqrt(t);
  }
}

struct Coefs { float coef, decay, omb1, b2, omb2, step_size, bc2_sqrt, eps; };

template <int MODE>
__device__ __forceinline__ void update_elem(float& p, float& g, float& m, float& v, const Coefs& k) {
#pragma clang fp contract(off)
  if (MODE != MODE_ADAMW) g = __fmul_rn(g, k.coef);
  if (MODE == MODE_CLIP) return;
  p = __fmul_rn(p, k.decay);
  m = __fadd_rn(m, __fmul_rn(__fsub_rn(g, m), k.omb1));
  v = __fadd_rn(__fmul_rn(v, k.b2), __fmul_rn(__fmul_rn(g, g), k.omb2));
  const float denom = __fadd_rn(__fdiv_rn(__fsqrt_rn(v), k.bc2_sqrt), k.eps);
  p = __fsub_rn(p, __fmul_rn(k.step_size, __fdiv_rn(m, denom)));
}

template <int MODE>
__device__ __forceinline__ void update_scalar(float* p, float* g, float* m, float* v, int e, const Coefs& k) {
  float pe = 0.f, ge = g[e], me = 0.f, ve = 0.f;
  if (MODE != MODE_CLIP) { pe = p[e]; me = m[e]; ve = v[e]; }
  update_elem<MODE>(pe, ge, me, ve, k);
  if (MODE != MODE_ADAMW) g[e] = ge;
  if (MODE != MODE_CLIP) { p[e] = pe; m[e] = me; v[e] = ve; }
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void multi_update_kernel(const MultiLaunch a) {
#pragma clang fp contract(off)
  __shared__ double s_red[kThreads / 64];
  __shared__ float s_coef;
  Coefs k;
  k.coef = 1.0f;
  if (MODE != MODE_ADAMW) {
    const double t = sum_partials(a.partials, a.npartials, s_red);
    if (threadIdx.x == 0) {
      const float total = (float)sqrt(t);
      s_coef = fminf(1.0f, __fdiv_rn(a.max_norm, __fadd_rn(total, 1e-6f)));
      if (a.total_out && blockIdx.x == 0) a.total_out[0] = total;
    }
    __syncthreads();
    k.coef = s_coef;
  }
  int i = 0;
  for (int c = blockIdx.x; c < a.nchunks; c += gridDim.x) {
    i = seg_of(a, c, i);
    const int64_t off = (int64_t)(c - a.seg[i].chunk0) * kChunk;
    const int64_t left = a.seg[i].numel - off;
    const int len = left < kChunk ? (int)left : kChunk;
    float* g = a.seg[i].g + off;
    float* p = nullptr; float* m = nullptr; float* v = nullptr;
    bool same = true;                              // do the four chunks reach a 16-byte boundary at the same element?
    if (MODE != MODE_CLIP) {
      p = a.seg[i].p + off; m = a.seg[i].m + off; v = a.seg[i].v + off;
      same = (((addr(p) ^ addr(g)) | (addr(m) ^ addr(g)) | (addr(v) ^ addr(g))) & 15) == 0;
      k.decay = a.seg[i].decay; k.omb1 = a.seg[i].omb1; k.b2 = a.seg[i].b2; k.omb2 = a.seg[i].omb2;
      k.step_size = a.seg[i].step_size; k.bc2_sqrt = a.seg[i].bc2_sqrt; k.eps = a.seg[i].eps;
    }
    const int head = head_of(g, len, same);
    const int nvec = (len - head) >> 2;
    for (int e = threadIdx.x; e < head; e += kThreads) update_scalar<MODE>(p, g, m, v, e, k);
    for (int q = threadIdx.x; q < nvec; q += kThreads) {
      const int e = head + 4 * q;
      float4 vg = *reinterpret_cast<const float4*>(g + e);
      float4 vp = {0, 0, 0, 0}, vm = vp, vv = vp;
      if (MODE != MODE_CLIP) {
        vp = *reinterpret_cast<const float4*>(p + e);
        vm = *reinterpret_cast<const float4*>(m + e);
        vv = *reinterpret_cast<const float4*>(v + e);
      }
      update_elem<MODE>(vp.x, vg.x, vm.x, vv.x, k);
      update_elem<MODE>(vp.y, vg.y, vm.y, vv.y, k);
      update_elem<MODE>(vp.z, vg.z, vm.z, vv.z, k);
      update_elem<MODE>(vp.w, vg.w, vm.w, vv.w, k);
      if (MODE != MODE_ADAMW) *reinterpret_cast<float4*>(g + e) = vg;
      if (MODE != MODE_CLIP) {
        *reinterpret_cast<float4*>(p + e) = vp;
        *reinterpret_cast<float4*>(m + e) = vm;
        *reinterpret_cast<float4*>(v + e) = vv;
      }
    }
    for (int e = head + 4 * nvec + threadIdx.x; e < len; e += kThreads) update_scalar<MODE>(p, g, m, v, e, k);
  }
}

inline int64_t chunks_of(int64_t numel) { return (numel + kChunk - 1) / kChunk; }

// the call's tensors cut into launches: every launch holds up to kMaxTensors segments and kMaxChunks chunks
struct Plan {
  std::vector<MultiLaunch> launches;
  int64_t chunks = 0;
};

void plan_add(Plan& pl, Seg s) {
  // a tensor with more than kMaxChunks chunks goes in as runs of whole chunks, each a segment of its own
  int64_t done = 0;
  while (done < s.numel) {
    if (pl.launches.empty() || pl.launches.back().nseg == kMaxTensors || pl.launches.back().nchunks == kMaxChunks) {
      MultiLaunch l{};
      l.partial0 = pl.chunks;
      pl.launches.push_back(l);
    }
    MultiLaunch& l = pl.launches.back();
    const int64_t room = (int64_t)(kMaxChunks - l.nchunks) * kChunk;
    const int64_t take = s.numel - done < room ? s.numel - done : room;
    Seg part = s;
    part.g = s.g + done;
    if (s.p) { part.p = s.p + done; part.m = s.m + done; part.v = s.v + done; }
    part.numel = take;
    part.chunk0 = l.nchunks;
    l.seg[l.nseg++] = part;
    l.nchunks += (int)chunks_of(take);
    pl.chunks += chunks_of(take);
    done += take;
  }
}

inline int grid_of(const MultiLaunch& l) { return l.nchunks < kMaxGrid ? l.nchunks : kMaxGrid; }

// norm pass (clip), finish where needed, update pass (mode >= 0; mode < 0: the norm alone)
int run_plan(Plan& pl, int mode, float max_norm, float* total_norm_dev, void* scratch, hipStream_t s) {
  double* sum = (double*)scratch;                  // scratch: the sum | one partial per chunk
  double* partials = sum + 1;
  const bool clip = mode != MODE_ADAMW;
  bool inline_sum = false;
  if (clip) {
    for (MultiLaunch& l : pl.launches) {
      l.partials = partials;
      LDMSEG_LAUNCH("grad_sumsq", grad_sumsq_kernel, dim3(grid_of(l)), dim3(kThreads), 0, s, l);
    }
    inline_sum = mode >= 0 && pl.launches.size() == 1 && pl.chunks <= kInlinePartials;
    if (!inline_sum)
      LDMSEG_LAUNCH("grad_norm_finish", grad_norm_finish_kernel, dim3(1), dim3(kThreads), 0, s, (const double*)partials, (int)pl.chunks,
                    sum, total_norm_dev);
  }
  if (mode < 0) return launch_status();
  for (MultiLaunch& l : pl.launches) {
    l.partials = inline_sum ? partials : sum;
    l.npartials = clip ? (inline_sum ? (int)pl.chunks : 1) : 0;
    l.max_norm = max_norm;
    l.total_out = (inline_sum && &l == &pl.launches.front()) ? total_norm_dev : nullptr;
    if (mode == MODE_CLIP) LDMSEG_LAUNCH("multi_update<clip>", multi_update_kernel<MODE_CLIP>, dim3(grid_of(l)), dim3(kThreads), 0, s, l);
    else if (mode == MODE_ADAMW) LDMSEG_LAUNCH("multi_update<adamw>", multi_update_kernel<MODE_ADAMW>, dim3(grid_of(l)), dim3(kThreads), 0, s, l);
    else LDMSEG_LAUNCH("multi_update<clip,adamw>", multi_update_kernel<MODE_CLIP_ADAMW>, dim3(grid_of(l)), dim3(kThreads), 0, s, l);
  }
  return launch_status();
}

inline bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

// the checks and the launches behind the three entries.  params NULL: gradients only (mode < 0 the norm, MODE_CLIP the clip)
int multi_tensor_entry(int n, float* const* params, float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                       const int64_t* numels, const ldmseg_adamw_hyper* hyper, int mode, float max_norm, float* total_norm_dev,
                       void* scratch, void* stream) {
  using namespace rt;
  g_err.clear();
  const bool update = mode == MODE_ADAMW || mode == MODE_CLIP_ADAMW;
  if (n < 0 || !grads || !numels || (update && (!params || !exp_avg || !exp_avg_sq || !hyper))) return fail(LDMSEG_E_ARG, "null argument");
  if (mode != MODE_ADAMW && (!total_norm_dev || !scratch)) return fail(LDMSEG_E_ARG, "the norm needs total_norm_dev and scratch");
  if (mode == MODE_CLIP && !(max_norm > 0.0f)) return fail(LDMSEG_E_ARG, "max_norm must be positive");
  if (!aligned4(total_norm_dev) || ((uintptr_t)scratch & 7)) return fail(LDMSEG_E_ARG, "total_norm_dev / scratch misaligned");
  Plan pl;
  for (int i = 0; i < n; ++i) {
    const std::string at = " (tensor " + std::to_string(i) + ")";
    if (numels[i] < 0) return fail(LDMSEG_E_ARG, "negative numel" + at);
    if (!aligned4(grads[i])) return fail(LDMSEG_E_ARG, "gradient not 4-byte aligned" + at);
    if (!grads[i] || numels[i] == 0) continue;     // no gradient: skipped wholly; nothing to do for an empty tensor
    Seg sg{};
    sg.g = grads[i];
    sg.numel = numels[i];
    if (update) {
      if (!params[i] || !exp_avg[i] || !exp_avg_sq[i]) return fail(LDMSEG_E_ARG, "null parameter / moment" + at);
      if (!aligned4(params[i]) || !aligned4(exp_avg[i]) || !aligned4(exp_avg_sq[i])) return fail(LDMSEG_E_ARG, "pointer not 4-byte aligned" + at);
      const ldmseg_adamw_hyper& h = hyper[i];
      if (h.step < 1) return fail(LDMSEG_E_ARG, "step must be >= 1: the count after this update" + at);
      if (!(h.beta1 >= 0.0 && h.beta1 < 1.0) || !(h.beta2 >= 0.0 && h.beta2 < 1.0)) return fail(LDMSEG_E_ARG, "betas must lie in [0, 1)" + at);
      if (!(h.lr >= 0.0) || !(h.eps >= 0.0) || !(h.weight_decay >= 0.0) || std::isinf(h.lr) || std::isinf(h.eps) || std::isinf(h.weight_decay))
        return fail(LDMSEG_E_ARG, "lr, eps and weight_decay must be finite and not negative" + at);
      sg.p = params[i]; sg.m = exp_avg[i]; sg.v = exp_avg_sq[i];
      const double bc1 = 1.0 - std::pow(h.beta1, (double)h.step), bc2 = 1.0 - std::pow(h.beta2, (double)h.step);
      sg.decay = (float)(1.0 - h.lr * h.weight_decay);
      sg.omb1 = (float)(1.0 - h.beta1);
      sg.b2 = (float)h.beta2;
      sg.omb2 = (float)(1.0 - h.beta2);
      sg.step_size = (float)(h.lr / bc1);
      sg.bc2_sqrt = (float)std::sqrt(bc2);
      sg.eps = (float)h.eps;
    }
    plan_add(pl, sg);
  }
  TRY(run_plan(pl, mode, max_norm, total_norm_dev, scratch, (hipStream_t)stream));
  return 0;
}

}  // namespace
}  // namespace ldmseg

using namespace ldmseg;

extern "C" {

size_t ldmseg_multi_tensor_scratch_bytes(int n, const int64_t* numels) {
  if (n < 0 || !numels) return 0;
  int64_t chunks = 0;
  for (int i = 0; i < n; ++i) {
    if (numels[i] < 0) return 0;
    chunks += chunks_of(numels[i]);
  }
  return (size_t)(1 + chunks) * sizeof(double);
}

int ldmseg_grad_norm(int n, const float* const* grads, const int64_t* numels, float* total_norm_dev, void* scratch, void* stream) {
  return multi_tensor_entry(n, nullptr, (float* const*)grads, nullptr, nullptr, numels, nullptr, -1, 0.f, total_norm_dev, scratch, stream);
}

int ldmseg_grad_clip(int n, float* const* grads, const int64_t* numels, float max_norm, float* total_norm_dev, void* scratch,
                     void* stream) {
  return multi_tensor_entry(n, nullptr, grads, nullptr, nullptr, numels, nullptr, MODE_CLIP, max_norm, total_norm_dev, scratch, stream);
}

int ldmseg_adamw_step(int n, float* const* params, float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                      const int64_t* numels, const ldmseg_adamw_hyper* hyper, float max_norm, float* total_norm_dev, void* scratch,
                      void* stream) {
  return multi_tensor_entry(n, params, grads, exp_avg, exp_avg_sq, numels, hyper, max_norm > 0.0f ? MODE_CLIP_ADAMW : MODE_ADAMW,
                            max_norm, total_norm_dev, scratch, stream);
}

}  // extern "C"
