// Single-operator entry points with an fp32 boundary (ldmseg_op_*): the parity tests
// drive each gfx950 kernel in isolation through these, with torch ops as the reference.
// Not on the hot path: every call allocates and frees its own staging buffers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/ldmseg_hip.h"
#include "common.h"
#include "attn_plan.h"
#include "gn_plan.h"
#include "kernels.h"
#include "ln_plan.h"
#include "nearest_index.h"
#include "runtime.h"
#include "vae_bwd.h"

using namespace ldmseg;
using rt::bke;
using rt::esize;
using rt::rup;

// Counter region of the in-launch split-K finish for these handle-less launches: one per device, zeroed once.  The operator
// entry points are test support and run one launch at a time per device (a handle owns its own region).
static unsigned long long* op_cf_region() {
  static unsigned long long* r[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  if (!r[dev]) {
    void* q = nullptr;
    if (hipMalloc(&q, igemm_cf_bytes()) != hipSuccess) return nullptr;
    (void)hipMemset(q, 0, igemm_cf_bytes());
    r[dev] = (unsigned long long*)q;
  }
  return r[dev];
}

namespace {

template <typename T>
__global__ void unpack_nhwc_kernel(const T* x, float* y, int C, int HW, int ldx) {
  const int pix = blockIdx.x * blockDim.x + threadIdx.x;
  const int img = blockIdx.y;
  if (pix >= HW) return;
  const T* r = x + ((size_t)img * HW + pix) * ldx;
  for (int c = 0; c < C; ++c) y[((size_t)img * C + c) * HW + pix] = to_f32<T>(r[c]);
}
template <typename T>
__global__ void convert_rows_kernel(const float* x, T* y, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) y[i] = from_f32<T>(x[i]);
}
template <typename T>
__global__ void convert_back_kernel(const T* x, float* y, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) y[i] = to_f32<T>(x[i]);
}
__global__ void fastdiv_probe_kernel(const int* n, int count, FastDiv f, int* q) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) q[i] = fd_div(n[i], f);
}
inline int rows_grid(size_t n) { return (int)std::min<size_t>(4096, std::max<size_t>(1, (n + 255) / 256)); }
// source rows of a packed GEGLU projection of nout outputs (geglu_row_map), zero rows (-1) behind them up to Np
std::vector<int> geglu_rows(int nout, int Np) {
  std::vector<int> map = geglu_row_map(nout);
  map.resize(Np, -1);
  return map;
}

// The staging of one call: its stream, its compute mode, its temporary device buffers and a sticky status.  The first failure
// sets the status - LDMSEG_E_OOM for a failed hipMalloc, -3 for a failed staging launch or copy - and every later operation
// does nothing and returns null.  An entry point tests `status` once, before the first launch of the kernel under test: past
// that test no staging pointer is null.  The destructor waits for the device and frees the buffers.
struct Stage {
  hipStream_t s;
  int dt;             // storage dtype, as the launchers take it
  int x3 = 0;         // split-bf16 products on fp32 tensors: 1 = weights split in the K loop, 2 = weights as hi | lo planes
  int status = 0;
  std::vector<void*> v;
  // split_modes: the entry point takes dtype 2 / 3 as the split-bf16 modes (otherwise dtype goes to the launchers as it is)
  Stage(void* stream, int dtype, bool split_modes = false) : s((hipStream_t)stream), dt(dtype) {
    if (split_modes) x3 = dtype == 2 ? 1 : (dtype == 3 ? 2 : 0);
    if (x3) dt = DT_F32;
  }
  ~Stage() {
    (void)hipDeviceSynchronize();
    for (void* p : v) (void)hipFree(p);
  }
  // a staging launch or copy: run unless the call has failed already, nonzero = failed
  template <typename F>
  void step(F launch) {
    if (!status && launch()) status = -3;
  }
  void* buf(size_t bytes) {
    if (status) return nullptr;
    void* p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) { status = LDMSEG_E_OOM; return nullptr; }
    v.push_back(p);
    return p;
  }
  // fp32 [n] -> compute dtype [n]
  void* rows(const float* x, size_t n) {
    void* y = buf(n * esize(dt));
    step([&] {
      if (dt == DT_BF16) hipLaunchKernelGGL(convert_rows_kernel<bf16_t>, dim3(rows_grid(n)), dim3(256), 0, s, x, (bf16_t*)y, n);
      else hipLaunchKernelGGL(convert_rows_kernel<float>, dim3(rows_grid(n)), dim3(256), 0, s, x, (float*)y, n);
      return hipGetLastError() != hipSuccess;
    });
    return status ? nullptr : y;
  }
  // NCHW fp32 [B, C, HW] -> NHWC compute dtype [B, HW, ld], channels C .. ld zero
  void* nchw(const float* x, int B, int C, int HW, int ld, float mul = 1.f, float add = 0.f) {
    void* y = buf((size_t)B * HW * ld * esize(dt));
    step([&] { return launch_pack_nchw(x, y, B, C, HW, ld, mul, add, dt, s); });
    return status ? nullptr : y;
  }
  // zero-padded [Npad] copy of a bias of n values (null: zeros)
  float* bias(const float* b, int n, int Npad) {
    float* y = (float*)buf(Npad * sizeof(float));
    step([&] { return launch_padded_bias(b, n, y, Npad, s); });
    return status ? nullptr : y;
  }
  // device copy of a host row map (a blocking copy: the vector may go away)
  int* ints(const std::vector<int>& map) {
    int* d = (int*)buf(map.size() * sizeof(int));
    step([&] { return hipMemcpy(d, map.data(), map.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess; });
    return status ? nullptr : d;
  }
  // device-to-device copy of n floats into a buffer of its own
  float* floats(const float* src, size_t n) {
    float* d = (float*)buf(n * sizeof(float));
    step([&] { return hipMemcpyAsync(d, src, n * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess; });
    return status ? nullptr : d;
  }
  // the way back: compute dtype [n] -> fp32 [n]
  int rows_out(const void* p, float* out, size_t n) {
    if (status) return status;
    if (dt == DT_BF16) hipLaunchKernelGGL(convert_back_kernel<bf16_t>, dim3(rows_grid(n)), dim3(256), 0, s, (const bf16_t*)p, out, n);
    else hipLaunchKernelGGL(convert_back_kernel<float>, dim3(rows_grid(n)), dim3(256), 0, s, (const float*)p, out, n);
    return launch_status();
  }
  // NHWC compute dtype [B, HW, ld] -> NCHW fp32 [B, C, HW]
  int nchw_out(const void* p, float* out, int B, int C, int HW, int ld) {
    if (status) return status;
    dim3 grid((HW + 255) / 256, B), block(256);
    if (dt == DT_BF16) hipLaunchKernelGGL(unpack_nhwc_kernel<bf16_t>, grid, block, 0, s, (const bf16_t*)p, out, C, HW, ld);
    else hipLaunchKernelGGL(unpack_nhwc_kernel<float>, grid, block, 0, s, (const float*)p, out, C, HW, ld);
    return launch_status();
  }
  // the split-K step of a launch that is filled in otherwise: `forced` K slices, or the engine's plan, and their partial sums
  void splitk(IgemmParams& p, int forced = 0) {
    if (status) return;
    const int splits = forced > 0 ? forced : igemm_plan_splits(p, dt), M = p.M, Np = p.N;
    if (splits > 1) { p.splits = splits; p.partial = (float*)buf((size_t)splits * M * Np * sizeof(float)); }
  }
};

// A conv / Linear weight in the engine's packing: [Np][k * k][c0 + c1] in the compute dtype (hi | lo planes when x3 == 2) and
// the bias padded to Np.  pack_shape: the padded sizes alone (no device).
struct Packed {
  void* w = nullptr;
  float* bias = nullptr;
  int Np = 0, c0 = 0, c1 = 0;
};
Packed pack_shape(int dt, int Co, int Ci, int Ci2, int epi, int n_store) {
  Packed r;
  const int nreal = n_store > Co ? n_store : Co;
  r.Np = (int)rup(nreal, igemm_pick_bn(nreal, epi));
  r.c0 = (int)rup(Ci, bke(dt));
  r.c1 = Ci2 ? (int)rup(Ci2, bke(dt)) : 0;
  return r;
}
// w: fp32 OIHW [Co][Ci + Ci2][k][k] (a Linear: [N][K], k = 1), bias [Co] or null.  Ci2 > 0: the input is a channel concat whose
// first part is K-tile aligned (the caller checks), the second is padded.  epi = EPI_GEGLU: w rows are [value | gate], packed
// through geglu_row_map with the bias in the same order.  n_store > Co: explicit zero output channels.  cm: channel-major K order.
Packed pack_weights(Stage& st, const float* w, const float* bias, int Co, int Ci, int Ci2, int k, int epi, int n_store, bool cm) {
  Packed r = pack_shape(st.dt, Co, Ci, Ci2, epi, n_store);
  const int Np = r.Np, ct = r.c0 + r.c1, dt = st.dt;
  hipStream_t s = st.s;
  r.w = st.buf((size_t)Np * k * k * ct * esize(dt));
  r.bias = st.bias(epi == EPI_GEGLU ? nullptr : bias, Co, Np);
  if (epi == EPI_GEGLU) {
    const int* dmap = st.ints(geglu_rows(Co / 2, Np));
    st.step([&] { return launch_repack_rows(w, r.w, dmap, Np, ct, dt, s); });
    if (bias) st.step([&] { return launch_repack_rows(bias, r.bias, dmap, Np, 1, DT_F32, s); });
  } else {
    const float* src = w;
    if (Ci2) {   // rows of Ci + Ci2 channels -> rows of c0 + c1 with zeros behind (c0 == Ci)
      void* w_cat = st.buf((size_t)Co * ct * k * k * sizeof(float));
      st.step([&] {
        return hipMemsetAsync(w_cat, 0, (size_t)Co * ct * k * k * sizeof(float), s) != hipSuccess ||
               hipMemcpy2DAsync(w_cat, (size_t)ct * k * k * sizeof(float), w, (size_t)(Ci + Ci2) * k * k * sizeof(float),
                                (size_t)(Ci + Ci2) * k * k * sizeof(float), Co, hipMemcpyDeviceToDevice, s) != hipSuccess;
      });
      src = (const float*)w_cat;
    }
    st.step([&] { return launch_repack_conv(src, r.w, Co, Ci2 ? ct : Ci, k, k, Np, ct, dt, s, cm ? bke(dt) : 0); });
  }
  if (st.x3 == 2) st.step([&] { return launch_split_planes(r.w, (size_t)Np * k * k * ct, s); });
  return r;
}

// output size of a k x k conv on an H x W map, nearest-x2 upsampled first if `up`: a 3x3 stride-2 conv halves it, with pad 1
// (pad = -1) or with pad 0 and one zero row / column at the bottom / right (pad = 0)
void conv_out_size(int H, int W, int k, int stride, int up, int pad, int* Ho, int* Wo) {
  const int Hl = up ? 2 * H : H, Wl = up ? 2 * W : W;
  const bool half = k == 3 && stride == 2;
  *Ho = !half ? Hl : (pad == 0 ? Hl / 2 : (Hl - 1) / 2 + 1);
  *Wo = !half ? Wl : (pad == 0 ? Wl / 2 : (Wl - 1) / 2 + 1);
}

// `warm` untimed calls of fn(i), then `iters` timed ones (i keeps counting) between two HIP events on `s`: microseconds per call
template <typename F>
float time_launches(hipStream_t s, int warm, int iters, F fn) {
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  for (int i = 0; i < warm; ++i) fn(i);
  (void)hipEventRecord(e0, s);
  for (int i = 0; i < iters; ++i) fn(warm + i);
  (void)hipEventRecord(e1, s);
  (void)hipEventSynchronize(e1);
  float ms = 0;
  (void)hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  return 1e3f * ms / iters;
}

int gn_plan_out(int r, const GnPlan& pl, int dtype, char* buf, int n) {
  if (!buf || n < 1) return -2;
  if (r == 0) std::snprintf(buf, (size_t)n, "%s", gn_plan_line(pl, dtype).c_str());
  return r;
}

// -2 where the attention launcher of `kind` has no launch for the shape (the chooser it asks; no device)
int attn_refused(int kind, int B, int N, int S, int C, int heads, int dtype) {
  AttnPlan pl;
  return attn_choose(AttnDesc{kind, B, N, S, C, heads, dtype}, attention_knobs(), &pl) ? -2 : 0;
}

// The engine's launch of one conv / GEMM layer, exactly as engine.hip issues it in a forward: NHWC operands in the compute
// dtype, the split-K plan of igemm_plan_splits (splits = 0) or a forced one, the row-major store epilogue with optional
// bias, per-image bias row (time embedding), residual and SiLU, or the GEGLU epilogue.  Boundary tensors are NCHW f32:
// x [B,Ci,H,W], x2 [B,Ci2,H,W] or NULL, w [Co,Ci+Ci2,k,k], resid [B,Cout,Ho,Wo] or NULL, rowbias [B,Co] or NULL,
// out [B,Cout,Ho,Wo] with Cout = Co (Co/2 for GEGLU, whose w rows are [value | gate] like ff.net.0.proj).
int g_bench_rot = 1, g_bench_ln = 0;
int op_igemm_impl(const float* x, const float* x2, const float* w, const float* bias, const float* resid,
                  const float* rowbias, int B, int Ci, int Ci2, int H, int W, int Co, int k, int stride, int up, int geglu,
                  int silu, int splits, int dtype, float* out, void* stream, int time_iters, float* us_per_launch) {
  Stage st(stream, dtype, true);   // LDMSEG_BF16X3: fp32 storage, split-bf16 products; 3 = the same with the weights
  dtype = st.dt;                   // split into hi | lo planes up front, as the handles hold them (round 6)
  hipStream_t s = st.s;
  const int a = bke(dtype);
  if (Ci2 && (Ci % a)) return -2;
  if (geglu && (k != 1 || Ci2 || (Co % 128))) return -2;   // (the GEGLU epilogue stores whole 128-column tiles: 64 outputs each)
  const int epi = geglu ? EPI_GEGLU : EPI_STORE;
  const int cout = geglu ? Co / 2 : Co;
  const Packed sh = pack_shape(dtype, Co, Ci, Ci2, epi, 0);
  const int c0 = sh.c0, c1 = sh.c1, ct = c0 + c1, Np = sh.Np;
  const bool cm = !geglu && igemm_conv_cm(H * W, ct, Np, k, stride, up, dtype) && (Ci % a) == 0 && (!Ci2 || (Ci2 % a) == 0);   // the engine's rule
  const Packed wk = pack_weights(st, w, bias, Co, Ci, Ci2, k, epi, 0, cm);
  IgemmParams p;
  p.src0 = st.nchw(x, B, Ci, H * W, c0); p.C0 = c0;
  p.src1 = Ci2 ? st.nchw(x2, B, Ci2, H * W, c1) : nullptr; p.C1 = c1;
  p.B = B; p.Hi = H; p.Wi = W; p.taps = k * k; p.stride = stride; p.up = up; p.cm = cm ? 1 : 0;
  conv_out_size(H, W, k, stride, up, -1, &p.Ho, &p.Wo);
  const int Ho = p.Ho, Wo = p.Wo;
  p.M = B * Ho * Wo; p.N = Np; p.n_valid = cout; p.W = wk.w; p.bias = wk.bias;
  p.rowbias = rowbias; p.rb_stride = Co;
  p.resid = resid ? st.nchw(resid, B, cout, Ho * Wo, cout) : nullptr; p.ldr = cout;
  void* op = st.buf((size_t)B * Ho * Wo * cout * esize(dtype));
  p.out = op; p.ldo = cout; p.epi = epi; p.silu = silu;
  p.x3 = st.x3;
  if (up && k == 3 && stride == 1 && !Ci2 && !geglu && !resid && !rowbias && !silu && igemm_up4_ok(B, H, W, c0, Np, dtype) && Ci == c0) {
    // the engine's form of an upsampler conv: four 2x2 phase convs on the low-resolution map (IgemmParams::up4)
    void* w4 = st.buf((size_t)16 * Np * c0 * esize(dtype));
    st.step([&] { return launch_pack_up4(w, w4, Co, Ci, Np, c0, dtype, s); });
    p.W = w4; p.taps = 4; p.up = 0; p.up4 = 1; p.Ho = H; p.Wo = W; p.M = 4 * B * H * W; p.cm = 0;
  }
  p.cf_ctr = op_cf_region();
  st.splitk(p, splits);
  if (time_iters > 0 && g_bench_ln && p.splits <= 1 && !rowbias) {   // time the folded-LayerNorm instantiation (mean 0, rstd 1, c1 0)
    float* stats = (float*)st.buf((size_t)p.M * 2 * sizeof(float));
    float* c1z = (float*)st.buf(Np * sizeof(float));
    std::vector<float> h((size_t)p.M * 2);
    for (int m = 0; m < p.M; ++m) { h[2 * m] = 0.f; h[2 * m + 1] = 1.f; }
    st.step([&] {
      return hipMemsetAsync(c1z, 0, Np * sizeof(float), s) != hipSuccess ||
             hipMemcpy(stats, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess;
    });
    p.rowstats = stats; p.c1 = c1z;
  }
  if (st.status) return st.status;
  const int r = launch_igemm(p, dtype, s);
  if (r) return r;
  if (time_iters > 0 && us_per_launch) {        // kernel timing (tools/): launches back to back on the stream, HIP events around
    // the weights of a layer are cold in the real forward (1.6 GB of them stream through per step): rotate over copies
    const size_t wbytes = p.up4 ? (size_t)16 * Np * c0 * esize(dtype) : (size_t)Np * k * k * ct * esize(dtype);
    const void* wsrc = p.W;                       // (the up4 launch reads its own packing)
    int rot = g_bench_rot < 1 ? 1 : g_bench_rot;
    std::vector<const void*> wc(1, wsrc);
    for (int i = 1; i < rot; ++i) {
      void* c = nullptr;                          // (a copy that does not fit shortens the rotation and fails nothing)
      if (hipMalloc(&c, wbytes) != hipSuccess) break;
      st.v.push_back(c);
      (void)hipMemcpyAsync(c, wsrc, wbytes, hipMemcpyDeviceToDevice, s);
      wc.push_back(c);
    }
    rot = (int)wc.size();
    *us_per_launch = time_launches(s, 3, time_iters, [&](int i) { p.W = wc[i % rot]; (void)launch_igemm(p, dtype, s); });
  }
  if (!out) return 0;
  return st.nchw_out(op, out, B, cout, Ho * Wo, cout);
}

// F.linear(F.layer_norm(x, (K,), gamma, beta, eps), w, bias) - or the GEGLU feed-forward half on the normalised input when
// geglu = 1 - computed the way the engine computes norm1 -> q|k|v and norm3 -> ff.net.0: statistics pass + GEMM on the raw x
// with the LayerNorm folded into weights and epilogue (IgemmParams::rowstats).  x [M,K], w [N,K], out [M, N or N/2], f32.
// silu: the SiLU flag of the store epilogue on top (the CLIP vision executor's layer_norm2 -> fc1).  A non-GEGLU N that is no
// multiple of 160 is padded with zero rows to the 160-column tile of the folded instantiations, in every mode - what the CLIP
// vision executor does for its N = 3 C and 4 C (before, such an N returned -2 except in the split-bf16 modes, where an
// N % 128 == 0 took the 128-column plain-loop form).
int op_ln_linear_impl(const float* x, const float* gamma, const float* beta, const float* w, const float* bias, int M, int K,
                      int N, float eps, int geglu, int silu, int dtype, float* out, void* stream) {
  Stage st(stream, dtype, true);   // LDMSEG_BF16X3 (3: weights pre-split into planes)
  dtype = st.dt;
  hipStream_t s = st.s;
  if (K % bke(dtype) || (geglu && N % 128)) return -2;
  void* xp = st.rows(x, (size_t)M * K);
  const int epi = geglu ? EPI_GEGLU : EPI_STORE;
  const int bn = (!geglu && N % 160 != 0) ? 160 : igemm_pick_bn(N, epi);     // (the folded instantiations: 160 columns, GEGLU 128)
  const int Np = (int)rup(N, bn);
  const int nout = geglu ? N / 2 : N;
  std::vector<int> map;
  if (geglu) map = geglu_rows(nout, Np);
  LnFold f;
  f.w[0] = w; f.bias[0] = bias; f.Nper = N; f.K = K; f.Npad = Np; f.gamma = gamma; f.beta = beta; f.dtype = dtype;
  if (geglu) f.row_map = &map;
  void* wp = st.buf((size_t)Np * K * esize(dtype));
  float* c1 = (float*)st.buf(Np * sizeof(float));
  float* c2 = (float*)st.buf(Np * sizeof(float));
  void* scratch = st.buf(ln_fold_scratch_bytes(f));
  st.step([&] { return launch_ln_fold(f, scratch, wp, c1, c2, s); });
  float* stats = (float*)st.buf((size_t)M * 2 * sizeof(float));
  st.step([&] { return launch_rowstats(xp, stats, M, K, eps, dtype, s); });
  void* op = st.buf((size_t)M * nout * esize(dtype));
  IgemmParams p;
  p.src0 = xp; p.C0 = K; p.B = 1; p.Hi = p.Ho = M; p.Wi = p.Wo = 1;
  p.M = M; p.N = Np; p.n_valid = nout; p.W = wp; p.bias = c2; p.rowstats = stats; p.c1 = c1;
  p.out = op; p.ldo = nout; p.epi = epi; p.silu = silu;
  p.x3 = st.x3;
  if (st.x3 == 2) st.step([&] { return launch_split_planes(wp, (size_t)Np * K, s); });      // (c1 / c2 above were taken from the fp32 matrix)
  st.splitk(p);
  if (st.status) return st.status;
  const int r = launch_igemm(p, dtype, s);
  if (r) return r;
  return st.rows_out(op, out, (size_t)M * nout);
}

// The entry of a transformer on caller-supplied weights: h = x Wp^T + bp (proj_in as a Linear on [M][C] rows), q|k|v = [Wq | Wk | Wv]
// LayerNorm(h; gamma, beta).  mode 0: the unfused launches (GEMM, row statistics, folded-LayerNorm GEMM); 1: the row-local fused
// kernel (tproj.hip; bf16, C = 320, M % 128 == 0).  Outputs fp32 h [M][C], qkv [M][3C].  time_iters > 0 also times the path.
int transformer_in_impl(const float* x, const float* gn_gamma, const float* gn_beta, float gn_eps, int gn_images, int gn_mode,
                        const float* wp, const float* bp, const float* gamma, const float* beta, const float* wq,
                        const float* wk, const float* wv, int M, int C, float eps, int dtype, int mode, float* h_out, float* qkv_out,
                        int time_iters, float* us_per_call, void* stream) {
  Stage st(stream, dtype);
  hipStream_t s = st.s;
  if (C % bke(dtype) || (mode != 0 && (dtype != DT_BF16 || !proj_qkv_stream_bytes(C) || M % 128))) return -2;
  // GroupNorm in front (gn_gamma != null; x = [gn_images][HW][C] rows): gn_mode 0 = a launch of its own, 1 = statistics pass + the
  // sweep inside the fused kernel (mode 1 only)
  GNParams gp;
  GnFold gf;
  void* xn = nullptr;
  if (gn_gamma) {
    if (gn_images < 1 || M % gn_images || C % 32 || (gn_mode == 1 && (mode != 1 || !proj_qkv_gn_fold_ok(M / gn_images)))) return -2;
    xn = st.buf((size_t)M * C * esize(dtype));
    float* gg = st.floats(gn_gamma, C);
    float* gb = st.floats(gn_beta, C);
    gp.C0 = C; gp.B = gn_images; gp.HW = M / gn_images; gp.groups = 32; gp.gamma = gg; gp.beta = gb; gp.eps = gn_eps; gp.silu = 0;
    gp.out = xn;
    gp.nchunk = gn_mode == 1 ? proj_qkv_gn_chunks(gp.B, gp.HW) : gn_nchunk(gp.B, gp.HW);
    gp.partial = (float*)st.buf((size_t)gp.B * gp.nchunk * 32 * 2 * sizeof(float));
    gf.partial = gp.partial; gf.gamma = gg; gf.beta = gb; gf.nchunk = gp.nchunk; gf.HW = gp.HW; gf.eps = gn_eps;
  }
  void* xp = st.rows(x, (size_t)M * C);
  void* hp = st.buf((size_t)M * C * esize(dtype));
  void* qp = st.buf((size_t)M * 3 * C * esize(dtype));
  void* wpp = st.rows(wp, (size_t)C * C);
  void* wqkv = st.buf((size_t)3 * C * C * esize(dtype));
  float* bias4 = (float*)st.buf((size_t)4 * C * sizeof(float));      // proj_in bias | W_q beta | W_k beta | W_v beta
  float* c1 = (float*)st.buf((size_t)3 * C * sizeof(float));
  st.step([&] { return hipMemcpyAsync(bias4, bp, C * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess; });
  LnFold f;
  f.parts = 3; f.w[0] = wq; f.w[1] = wk; f.w[2] = wv; f.Nper = C; f.K = C; f.Npad = 3 * C; f.gamma = gamma; f.beta = beta; f.dtype = dtype;
  void* scratch = st.buf(ln_fold_scratch_bytes(f));
  st.step([&] { return launch_ln_fold(f, scratch, wqkv, c1, bias4 + C, s); });
  void* stream_w = nullptr;
  if (mode != 0) {
    stream_w = st.buf(proj_qkv_stream_bytes(C));
    st.step([&] { return launch_pack_proj_qkv_stream(wpp, wqkv, stream_w, C, s); });
  }
  float* stats = (float*)st.buf((size_t)M * 2 * sizeof(float));
  st.step([&] { return igemm_warm(); });
  if (st.status) return st.status;
  auto gemm = [&](const void* src, const void* W, int N, const float* bias, void* o, const float* rs, const float* cc1) -> int {
    IgemmParams p;
    p.src0 = src; p.C0 = C; p.B = 1; p.Hi = p.Ho = M; p.Wi = p.Wo = 1;
    p.M = M; p.N = N; p.n_valid = N; p.W = W; p.bias = bias; p.rowstats = rs; p.c1 = cc1;
    p.out = o; p.ldo = N; p.epi = EPI_STORE;
    st.splitk(p);
    return st.status ? st.status : launch_igemm(p, dtype, s);
  };
  auto run = [&]() -> int {
    const void* xin = xp;
    if (gn_gamma) {
      gp.src0 = xp;
      if (gn_mode == 1) {
        if (int r = launch_groupnorm_stats(gp, dtype, s)) return r;
        return launch_proj_qkv_fused(xp, hp, qp, stream_w, bias4, igemm_zero_page(), M, C, eps, &gf, s);
      }
      if (int r = launch_groupnorm(gp, dtype, s)) return r;
      xin = xn;
    }
    if (mode == 0) {
      if (int r = gemm(xin, wpp, C, bias4, hp, nullptr, nullptr)) return r;
      if (int r = launch_rowstats(hp, stats, M, C, eps, dtype, s)) return r;
      return gemm(hp, wqkv, 3 * C, bias4 + C, qp, stats, c1);
    }
    return launch_proj_qkv_fused(xin, hp, qp, stream_w, bias4, igemm_zero_page(), M, C, eps, nullptr, s);
  };
  if (int r = run()) return r;
  if (time_iters > 0 && us_per_call) *us_per_call = time_launches(s, 2, time_iters, [&](int) { (void)run(); });
  if (int r = st.rows_out(hp, h_out, (size_t)M * C)) return r;
  return st.rows_out(qp, qkv_out, (size_t)M * 3 * C);
}

}  // namespace

namespace ldmseg {
void ops_bench_knob(int key, int value) {
  if (key == 6) g_bench_rot = value;
  if (key == 7) g_bench_ln = value;
}
}  // namespace ldmseg

extern "C" {

// F.conv2d(cat([x, x2], 1) [nearest-x2 upsampled if up], w, bias, stride, padding=k//2) ; NCHW f32 in/out
int ldmseg_op_conv2d(const float* x, const float* x2, const float* w, const float* bias, int B, int Ci, int Ci2, int H,
                     int W, int Co, int k, int stride, int up, int dtype, float* out, void* stream) {
  Stage st(stream, dtype, true);   // split-bf16 products on fp32 tensors (3: weights as hi | lo planes)
  dtype = st.dt;
  if (Ci2 && (Ci % bke(dtype))) return -2;  // a concat boundary must be K-tile aligned
  const Packed wk = pack_weights(st, w, bias, Co, Ci, Ci2, k, EPI_STORE, 0, false);
  IgemmParams p;
  p.src0 = st.nchw(x, B, Ci, H * W, wk.c0); p.C0 = wk.c0;
  p.src1 = Ci2 ? st.nchw(x2, B, Ci2, H * W, wk.c1) : nullptr; p.C1 = wk.c1;
  p.B = B; p.Hi = H; p.Wi = W; p.taps = k * k; p.stride = stride; p.up = up;
  conv_out_size(H, W, k, stride, up, -1, &p.Ho, &p.Wo);
  p.M = B * p.Ho * p.Wo; p.N = wk.Np; p.n_valid = Co; p.W = wk.w; p.bias = wk.bias; p.out = out; p.epi = EPI_NCHW_F32;
  p.x3 = st.x3;
  if (std::getenv("LDMSEG_OP_TIMING_NHWC")) {   // kernel-timing experiments: the engine's NHWC store epilogue (output discarded)
    p.out = st.buf((size_t)p.M * Co * esize(dtype)); p.ldo = Co; p.epi = EPI_STORE;
  }
  if (st.status) return st.status;
  return launch_igemm(p, dtype, st.s);
}

// out = a + b over n_segs tensors (see ldmseg_hip_ops.h for the guard layout)
int ldmseg_op_skip_add(const float* a, const float* b, const int64_t* seg_elems, int n_segs, int dtype, float* out, void* stream) {
  if (!a || !b || !seg_elems || !out || n_segs < 1 || n_segs > kSkipAddMaxSegs || (dtype != DT_F32 && dtype != DT_BF16)) return -2;
  Stage st(stream, dtype);
  constexpr int kGuard = 8;
  size_t total = 0;
  for (int k = 0; k < n_segs; ++k) {
    if (seg_elems[k] < 0) return -2;
    total += (size_t)seg_elems[k] + kGuard;
  }
  char* ap = (char*)st.rows(a, total);
  char* bp = (char*)st.rows(b, total);
  char* op = (char*)st.rows(out, total);
  if (st.status) return st.status;
  SkipAddSeg segs[kSkipAddMaxSegs];
  size_t off = 0;
  for (int k = 0; k < n_segs; ++k) {
    segs[k].dst = op + off * esize(dtype);
    segs[k].a = ap + off * esize(dtype);
    segs[k].b = bp + off * esize(dtype);
    segs[k].elems = (long long)seg_elems[k];
    off += (size_t)seg_elems[k] + kGuard;
  }
  const int r = launch_skip_add(segs, n_segs, dtype, st.s);
  if (r) return r;
  return st.rows_out(op, out, total);
}

// out = proj_out(h + ff.net.2(g)) + x  (diffusers BasicTransformerBlock.ff.net[2] + residual, Transformer2DModel.proj_out + residual;
// /root/reference/ldmseg/models/unet.py:401-425) exactly as the bf16 / fp32 engines launch it at the 640- / 1280-channel levels:
// chained matrix [Wp W2 | Wp] and bias bp + Wp b2 formed in fp32 by launch_chain_weights (the create-time kernel), packed to the
// compute dtype like TransformerW::ffp, then ONE two-source 1x1 igemm over [g | h] with x as the residual (the launch plan, K slices
// and instantiation are the engine's).  g [M][4C], h / x / out [M][C], w2 [C][4C], wp [C][C]; b2 / bp may be NULL.
int ldmseg_op_chained_ff_out(const float* g, const float* h, const float* x, const float* w2, const float* b2, const float* wp,
                             const float* bp, int M, int C, int rows_per_image, int dtype, float* out, void* stream) {
  Stage st(stream, dtype);
  if (C % bke(dtype) || M < 1 || rows_per_image < 1 || M % rows_per_image) return -2;
  if (pack_shape(dtype, C, 5 * C, 0, EPI_STORE, 0).Np != C) return -2;   // (640 and 1280 are multiples of the 160-column tile)
  float* wcat = (float*)st.buf((size_t)C * 5 * C * sizeof(float));
  float* bcat = (float*)st.buf((size_t)C * sizeof(float));
  st.step([&] { return launch_chain_weights(wp, w2, b2, bp, wcat, bcat, C, st.s); });
  const Packed wk = pack_weights(st, wcat, nullptr, C, 5 * C, 0, 1, EPI_STORE, 0, false);
  void* op = st.buf((size_t)M * C * esize(dtype));
  IgemmParams p;
  p.src0 = st.rows(g, (size_t)M * 4 * C); p.C0 = 4 * C; p.src1 = st.rows(h, (size_t)M * C); p.C1 = C;
  p.B = M / rows_per_image; p.Hi = p.Ho = rows_per_image; p.Wi = p.Wo = 1; p.taps = 1;
  p.M = M; p.N = wk.Np; p.n_valid = C; p.W = wk.w; p.bias = bcat;
  p.resid = st.rows(x, (size_t)M * C); p.ldr = C; p.out = op; p.ldo = C; p.epi = EPI_STORE;
  p.cf_ctr = op_cf_region();
  st.splitk(p);
  if (st.status) return st.status;
  const int r = launch_igemm(p, dtype, st.s);
  if (r) return r;
  return st.rows_out(op, out, (size_t)M * C);
}

// y = [silu]( x @ w^T + bias [+ rowbias[row / rows_per_image]] [+ resid] )   or GEGLU when geglu=1 (w is [2*Nout, K])
int ldmseg_op_linear(const float* x, const float* w, const float* bias, const float* resid, const float* rowbias,
                     int rows_per_image, int M, int K, int N, int geglu, int silu, int splits, int dtype, float* out,
                     void* stream) {
  Stage st(stream, dtype);
  if (K % bke(dtype) || (geglu && N % 128)) return -2;   // (the GEGLU epilogue stores whole 128-column tiles)
  const int epi = geglu ? EPI_GEGLU : EPI_STORE;
  const int nout = geglu ? N / 2 : N;
  const Packed wk = pack_weights(st, w, bias, N, K, 0, 1, epi, 0, false);
  void* op = st.buf((size_t)M * nout * esize(dtype));
  IgemmParams p;
  p.src0 = st.rows(x, (size_t)M * K); p.C0 = K; p.B = M / rows_per_image; p.Hi = p.Ho = rows_per_image; p.Wi = p.Wo = 1;
  p.M = M; p.N = wk.Np; p.n_valid = nout; p.W = wk.w; p.bias = wk.bias;
  p.rowbias = rowbias; p.rb_stride = N;
  p.resid = resid ? st.rows(resid, (size_t)M * N) : nullptr; p.ldr = N; p.out = op; p.ldo = nout; p.epi = epi; p.silu = silu;
  p.cf_ctr = op_cf_region();
  if (splits > 1) st.splitk(p, splits);   // (no plan of its own: one K slice unless asked)
  if (st.status) return st.status;
  const int r = launch_igemm(p, dtype, st.s);
  if (r) return r;
  return st.rows_out(op, out, (size_t)M * nout);
}

// F.group_norm(cat([x,x2],1), 32, gamma, beta, eps) [+SiLU]; NCHW f32 in/out
int ldmseg_op_groupnorm(const float* x, const float* x2, const float* gamma, const float* beta, int B, int C, int C2, int HW,
                        float eps, int silu, int dtype, float* out, void* stream) {
  if (B < 1 || C < 1 || C2 < 0 || HW < 1) return -2;
  Stage st(stream, dtype);
  GNParams g;
  g.src0 = st.nchw(x, B, C, HW, C); g.C0 = C; g.src1 = C2 ? st.nchw(x2, B, C2, HW, C2) : nullptr; g.C1 = C2;
  void* op = st.buf((size_t)B * HW * (C + C2) * esize(dtype));
  g.B = B; g.HW = HW; g.gamma = gamma; g.beta = beta; g.eps = eps;
  g.silu = silu; g.out = op; g.nchunk = gn_nchunk(B, HW);
  g.partial = (float*)st.buf((size_t)B * g.nchunk * 64 * sizeof(float));
  if (st.status) return st.status;
  const int r = launch_groupnorm(g, dtype, st.s);
  if (r) return r;
  return st.nchw_out(op, out, B, C + C2, HW, C + C2);
}

// silu(GroupNorm32(conv3x3(x, w, bias) + rowbias[image])) through the engine's fused path: the conv as `splits` K slices without
// its own finish, then launch_finish_groupnorm.  -4: the shape has no fused instantiation (the engine then runs conv and norm apart).
int ldmseg_op_conv_groupnorm(const float* x, const float* w, const float* bias, const float* rowbias, const float* gamma,
                             const float* beta, int B, int Ci, int H, int W, int Co, float eps, int silu, int splits, int dtype,
                             float* out, void* stream) {
  Stage st(stream, dtype);
  if (Ci % bke(dtype) || splits < 2) return -2;
  if (!finish_groupnorm_ok(B, H * W, Co, dtype)) return -4;
  const Packed wk = pack_weights(st, w, bias, Co, Ci, 0, 3, EPI_STORE, 0, false);
  void* op = st.buf((size_t)B * H * W * Co * esize(dtype));
  IgemmParams p;
  p.src0 = st.nchw(x, B, Ci, H * W, Ci); p.C0 = Ci; p.B = B; p.Hi = H; p.Wi = W; p.Ho = H; p.Wo = W; p.taps = 9;
  p.M = B * H * W; p.N = wk.Np; p.n_valid = Co; p.W = wk.w; p.bias = wk.bias; p.rowbias = rowbias; p.rb_stride = Co;
  p.epi = EPI_STORE; p.no_finish = 1;
  st.splitk(p, splits);
  if (st.status) return st.status;
  int r = launch_igemm(p, dtype, st.s);
  if (r) return r;
  GNParams g;
  g.C0 = Co; g.B = B; g.HW = H * W; g.gamma = gamma; g.beta = beta; g.eps = eps; g.silu = silu; g.out = op;
  r = launch_finish_groupnorm(p, g, dtype, st.s);
  if (r) return r;
  return st.nchw_out(op, out, B, Co, H * W, Co);
}

// The dispatch string of a described GroupNorm launch (gn_plan.h: the chooser under the current knobs; no device): the
// dispatch-log names joined by " + ", then " splits=S grid=GXxGY block=T" (two launches: grid=GXxGY+GXxGY); -2 where ldmseg_op_groupnorm returns -2.
// ldmseg_op_conv_groupnorm_plan: the finish + GroupNorm launch of ldmseg_op_conv_groupnorm; -4 where that returns -4.
int ldmseg_op_groupnorm_plan(int B, int C, int C2, int HW, int groups, int dtype, int cus, int region_ok, char* buf, int n) {
  GnPlan pl;
  return gn_plan_out(groupnorm_plan(GnDesc{B, HW, C, C2, groups, gn_nchunk(B, HW), dtype}, cus, region_ok != 0, &pl), pl, dtype, buf, n);
}
int ldmseg_op_conv_groupnorm_plan(int B, int Co, int HW, int dtype, char* buf, int n) {
  GnPlan pl;
  return gn_plan_out(finish_groupnorm_plan(B, HW, Co, dtype, &pl), pl, dtype, buf, n);
}

// The dispatch string of a described LayerNorm (stats = 0: ldmseg_op_layernorm) or row-statistics launch (stats = 1: the pass in
// front of a folded-LayerNorm GEMM) under the current debug key 8 (ln_plan.h; no device): the dispatch-log name, then
// " grid=GX block=T"; -2 where the launch returns -2.
int ldmseg_op_layernorm_plan(int M, int C, int dtype, int stats, char* buf, int n) {
  if (!buf || n < 1) return -2;
  LnPlan pl;
  const int r = layernorm_plan(LnDesc{M, C, dtype, stats}, &pl);
  if (r == 0) std::snprintf(buf, (size_t)n, "%s", ln_plan_line(pl, dtype).c_str());
  return r;
}

// timing of one GroupNorm launch shape the way the engine launches it (tools/kbench.py gn): average microseconds over
// `iters` back-to-back launches between two HIP events; the input is whatever the allocation holds (statistics of garbage
// cost the same), gamma / beta are [C + C2] device vectors
int ldmseg_bench_groupnorm(const float* gamma, const float* beta, int B, int C, int C2, int HW, int silu, int dtype, int iters,
                           float* us_per_launch, void* stream) {
  Stage st(stream, dtype);
  hipStream_t s = st.s;
  void* xp = st.buf((size_t)B * HW * C * esize(dtype));
  void* x2p = C2 ? st.buf((size_t)B * HW * C2 * esize(dtype)) : nullptr;
  void* op = st.buf((size_t)B * HW * (C + C2) * esize(dtype));
  st.step([&] { return hipMemsetAsync(xp, 0x3c, (size_t)B * HW * C * esize(dtype), s) != hipSuccess; });
  if (C2) st.step([&] { return hipMemsetAsync(x2p, 0x3c, (size_t)B * HW * C2 * esize(dtype), s) != hipSuccess; });
  GNParams g;
  g.src0 = xp; g.C0 = C; g.src1 = x2p; g.C1 = C2; g.B = B; g.HW = HW; g.gamma = gamma; g.beta = beta; g.eps = 1e-5f;
  g.silu = silu; g.out = op; g.nchunk = gn_nchunk(B, HW);
  g.partial = (float*)st.buf((size_t)B * g.nchunk * 64 * sizeof(float));
  if (st.status) return st.status;
  int err = 0;
  *us_per_launch = time_launches(s, 3, iters, [&](int) { if (const int r = launch_groupnorm(g, dtype, s)) err = err ? err : r; });
  return err;
}

// The fused evaluation tail (ldmseg_vae_decode_panoptic) on a given 4L decoder output x4 [B,C,H4,W4] f32 NCHW: packs it to
// NHWC `dtype` and runs the resample + scan / filter / remap kernels.  volume (optional) receives the resampled logits
// [C][h_b * w_b] of every image back to back (image b at C * offsets[b]) so that the interpolation chain itself can be
// compared with F.interpolate o crop o F.interpolate.
int ldmseg_op_panoptic_from_decoder(const float* x4, int B, int C, int H4, int W4, int dtype, int in_h, int in_w,
                                    const int32_t* boxes, const int32_t* sizes, const int64_t* offsets, int threshold_output,
                                    int threshold_mode, float mask_th, int count_th, double overlap_th, int64_t ignore_label,
                                    int32_t* labels, int32_t* panoptic, uint8_t* keep, int32_t* counts, int32_t* mask_counts,
                                    float* volume, void* stream) {
  Stage st(stream, dtype);
  void* xp = st.nchw(x4, B, C, H4 * W4, C);
  if (st.status) return st.status;
  return launch_panoptic_from_decoder(xp, B, H4, W4, C, dtype, in_h, in_w, boxes, sizes, offsets, threshold_output,
                                      threshold_mode, mask_th, count_th, overlap_th, ignore_label, labels, panoptic, keep, counts,
                                      mask_counts, st.s, volume);
}

// The fused mIoU tail (ldmseg_vae_decode_semseg) on a given 4L decoder output x4 [B,C,H4,W4] f32 NCHW: packs it to NHWC `dtype`
// and runs semseg_scan_kernel.  volume (optional) receives the resampled logits [B][C][out_h * out_w] so that the interpolation
// itself can be compared with F.interpolate(align_corners=True).
int ldmseg_op_semseg_from_decoder(const float* x4, int B, int C, int H4, int W4, int dtype, int out_h, int out_w, float mask_th,
                                  int64_t ignore_label, const int64_t* targets, int64_t ignore_index, int num_classes,
                                  int64_t* preds, int64_t* counts, float* volume, void* stream) {
  if (!x4 || B < 1 || C < 1 || H4 < 1 || W4 < 1) return -2;
  Stage st(stream, dtype);
  void* xp = st.nchw(x4, B, C, H4 * W4, C);
  if (st.status) return st.status;
  return launch_semseg_from_decoder(xp, B, H4, W4, C, dtype, out_h, out_w, mask_th, ignore_label, targets, ignore_index, num_classes,
                                    preds, counts, st.s, volume);
}

int ldmseg_op_layernorm(const float* x, const float* gamma, const float* beta, int M, int C, float eps, int silu, int dtype,
                        float* out, void* stream) {
  if (M < 1 || C < 1) return -2;
  Stage st(stream, dtype);
  void* xp = st.rows(x, (size_t)M * C);
  if (st.status) return st.status;
  const int r = launch_layernorm(xp, xp, gamma, beta, M, C, eps, silu, dtype, st.s);
  if (r) return r;
  return st.rows_out(xp, out, (size_t)M * C);
}

// softmax(q k^T d^-0.5) v per head on fused qkv [B,N,3C] f32 -> [B,N,C] f32
int ldmseg_op_attention(const float* qkv, int B, int N, int C, int heads, int dtype, float* out, void* stream) {
  if (attn_refused(ATTN_KIND_SELF, B, N, 0, C, heads, dtype)) return -2;
  Stage st(stream, dtype);
  void* qp = st.rows(qkv, (size_t)B * N * 3 * C);
  void* op = st.buf((size_t)B * N * C * esize(dtype));
  if (st.status) return st.status;
  const int r = launch_attention(qp, op, B, N, C, heads, dtype, st.s);
  if (r) return r;
  return st.rows_out(op, out, (size_t)B * N * C);
}

// The dispatch string of a described attention launch (attn_plan.h: the chooser under the current debug keys 2 and 15; no
// device): kind 0 = ldmseg_op_attention, 1 = _causal, 2 = _fp8, 3 = _cross (S: context rows, otherwise ignored); per launch
// "name grid=.. block=..", the pre-pass of the fp8 forms first, joined by " + ".  -2 where the operator returns -2.
int ldmseg_op_attention_plan(int kind, int B, int N, int S, int C, int heads, int dtype, char* buf, int n) {
  if (!buf || n < 1) return -2;
  AttnPlan pl;
  const int r = attn_choose(AttnDesc{kind, B, N, S, C, heads, kind == ATTN_KIND_FP8 ? (int)DT_BF16 : dtype}, attention_knobs(), &pl);
  if (r == 0) std::snprintf(buf, (size_t)n, "%s", attn_plan_line(pl).c_str());
  return r;
}

int ldmseg_op_attention_causal(const float* qkv, int B, int N, int C, int heads, int dtype, float* out, void* stream) {
  if (B < 1 || N < 1 || heads < 1 || C != 64 * heads) return -2;
  Stage st(stream, dtype);
  void* qp = st.rows(qkv, (size_t)B * N * 3 * C);
  void* op = st.buf((size_t)B * N * C * esize(dtype));
  if (st.status) return st.status;
  const int r = launch_attention_causal(qp, op, B, N, C, heads, dtype, st.s);
  if (r) return r;
  return st.rows_out(op, out, (size_t)B * N * C);
}

int ldmseg_op_clip_text_tokens(const int64_t* ids, const float* tok, const float* pos, int R, int T, int C, int vocab, int dtype,
                               float* out, void* stream) {
  if (R < 1 || T < 1 || C < 1 || vocab < 1) return -2;
  Stage st(stream, dtype);
  void* hp = st.buf((size_t)R * T * C * esize(dtype));
  if (st.status) return st.status;
  const int r = launch_clip_text_tokens(ids, tok, pos, hp, R, T, C, vocab, dtype, st.s);
  if (r) return r;
  return st.rows_out(hp, out, (size_t)R * T * C);
}

int ldmseg_op_clip_text_final_ln(const float* x, const float* gamma, const float* beta, int M, int C, float eps, int dtype,
                                 float* out, void* stream) {
  if (M < 1 || C < 1) return -2;
  Stage st(stream, dtype);
  void* xp = st.rows(x, (size_t)M * C);
  if (st.status) return st.status;
  return launch_clip_text_final_ln(xp, gamma, beta, out, M, C, eps, dtype, st.s);
}

int ldmseg_op_attention_cross(const float* q, const float* kv, int B, int N, int S, int C, int heads, int dtype, float* out,
                              void* stream) {
  if (B < 1 || N < 1 || S < 1 || heads < 1 || C % heads) return -2;
  Stage st(stream, dtype);
  void* qp = st.rows(q, (size_t)B * N * C);
  void* kp = st.rows(kv, (size_t)B * S * 2 * C);
  void* op = st.buf((size_t)B * N * C * esize(dtype));
  if (st.status) return st.status;
  const int r = launch_attention_cross(qp, kp, op, B, N, S, C, heads, dtype, st.s);
  if (r) return r;
  return st.rows_out(op, out, (size_t)B * N * C);
}

// ConvTranspose2d(k=2,s=2): x NCHW f32 [B,Ci,H,W], w [Ci,Co,2,2] -> NCHW f32 [B,Co,2H,2W]
int ldmseg_op_convt2(const float* x, const float* w, const float* bias, int B, int Ci, int H, int W, int Co, int dtype,
                     float* out, void* stream) {
  Stage st(stream, dtype, true);   // split-bf16 products on fp32 tensors (3: weights as hi | lo planes, as a bf16x3 handle)
  dtype = st.dt;
  hipStream_t s = st.s;
  if (Ci % bke(dtype) || Co % 4) return -2;
  const int N = 4 * Co;
  const int Np = pack_shape(dtype, N, Ci, 0, EPI_STORE, 0).Np;
  void* wp = st.buf((size_t)Np * Ci * esize(dtype));
  float* bp = st.bias(nullptr, 0, Np);
  st.step([&] {
    if (hipMemsetAsync(wp, 0, (size_t)Np * Ci * esize(dtype), s) != hipSuccess || launch_repack_convt2(w, wp, Ci, Co, dtype, s)) return true;
    for (int q = 0; bias && q < 4; ++q)
      if (hipMemcpyAsync(bp + q * Co, bias, Co * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) return true;
    return st.x3 == 2 && launch_split_planes(wp, (size_t)Np * Ci, s) != 0;
  });
  void* op = st.buf((size_t)B * 4 * H * W * Co * esize(dtype));
  IgemmParams p;
  p.src0 = st.nchw(x, B, Ci, H * W, Ci); p.C0 = Ci; p.B = B; p.Hi = p.Ho = H; p.Wi = p.Wo = W; p.M = B * H * W; p.N = Np; p.n_valid = N;
  p.W = wp; p.bias = bp; p.out = op; p.ldo = Co; p.epi = EPI_CONVT2; p.cout = Co;
  p.x3 = st.x3;
  if (st.status) return st.status;
  const int r = launch_igemm(p, dtype, s);
  if (r) return r;
  return st.nchw_out(op, out, B, Co, 4 * H * W, Co);
}

// ---- the launch forms of the two VAEs (vae.hip), each with IgemmParams filled the way the model fills them
// One conv the way Exec::conv / the VAE heads launch it: the `pad` argument of the stride-2 convs (-1: pad 1 both sides; 0: pad 0 +
// one zero row / column at the bottom / right, Ho = H / 2), SiLU and residual in the store epilogue, `n_store` > Co = explicit zero
// output channels up to the next layer's K tile (Builder::conv), epi = EPI_STORE or EPI_NCHW_F32 (the 8-channel heads and the
// logits).  No channel-major packing and no extra tap: the VAE builders make neither.
int ldmseg_op_vae_conv(const float* x, const float* w, const float* bias, const float* resid, int B, int Ci, int H, int W, int Co, int k,
                       int stride, int pad, int silu, int epi, int n_store, int dtype, float* out, void* stream) {
  Stage st(stream, dtype, true);
  dtype = st.dt;
  if (!x || !w || !out || B < 1 || Ci < 1 || Co < 1 || H < 1 || W < 1 || (k != 1 && k != 3) || (stride != 1 && stride != 2) ||
      (pad != -1 && pad != 0) || (pad == 0 && (k != 3 || stride != 2)) || (epi != EPI_STORE && epi != EPI_NCHW_F32) ||
      (epi == EPI_NCHW_F32 && (resid || silu)))
    return -2;
  const int nreal = n_store > Co ? n_store : Co;
  int Ho, Wo;
  conv_out_size(H, W, k, stride, 0, pad, &Ho, &Wo);
  if (Ho < 1 || Wo < 1) return -2;
  const Packed wk = pack_weights(st, w, bias, Co, Ci, 0, k, epi, n_store, false);
  IgemmParams p;
  p.src0 = st.nchw(x, B, Ci, H * W, wk.c0); p.C0 = wk.c0;
  p.B = B; p.Hi = H; p.Wi = W; p.Ho = Ho; p.Wo = Wo;
  p.taps = k * k; p.stride = stride; p.pad = pad;
  p.M = B * Ho * Wo; p.N = wk.Np; p.W = wk.w; p.bias = wk.bias;
  p.x3 = st.x3;
  p.cf_ctr = op_cf_region();
  void* op = nullptr;
  if (epi == EPI_NCHW_F32) {
    p.n_valid = Co; p.out = out; p.epi = EPI_NCHW_F32;
  } else {
    op = st.buf((size_t)B * Ho * Wo * nreal * esize(dtype));
    p.n_valid = nreal; p.out = op; p.ldo = nreal; p.epi = EPI_STORE; p.silu = silu;
    if (resid) { p.resid = st.nchw(resid, B, Co, Ho * Wo, nreal); p.ldr = nreal; }
  }
  st.splitk(p);
  if (st.status) return st.status;
  const int r = launch_igemm(p, dtype, st.s);
  if (r || epi == EPI_NCHW_F32) return r;
  return st.nchw_out(op, out, B, Co, Ho * Wo, nreal);
}

// out [M][N] = a [M][K] b[N][K]^T (+ bias[N]): both operands are activations (klenc_attention: S = Q K^T, V^T = W_v X^T, O = P V + b_v),
// so W is taken as it is (w_dynamic) and a split-bf16 mode splits it in the K loop (dtype 2 and 3 both run x3 = 1, as Exec::igemm
// sets it).  rows_f32: EPI_ROWS_F32 (fp32 rows whatever the compute dtype), else the store epilogue.
int ldmseg_op_gemm_dynamic(const float* a, const float* b, const float* bias, int M, int N, int K, int rows_f32, int dtype, float* out,
                           void* stream) {
  Stage st(stream, dtype, true);
  dtype = st.dt;
  if (!a || !b || !out || M < 1 || N < 1 || K < 1 || K % bke(dtype) || N % 32) return -2;
  void* op = rows_f32 ? nullptr : st.buf((size_t)M * N * esize(dtype));
  IgemmParams p;
  p.src0 = st.rows(a, (size_t)M * K); p.C0 = K; p.B = 1; p.Hi = p.Ho = M; p.Wi = p.Wo = 1;
  p.M = M; p.N = N; p.n_valid = N; p.W = st.rows(b, (size_t)N * K); p.bias = bias; p.ldo = N;
  p.out = rows_f32 ? (void*)out : op; p.epi = rows_f32 ? EPI_ROWS_F32 : EPI_STORE;
  p.w_dynamic = 1;
  p.x3 = st.x3 ? 1 : 0;
  p.cf_ctr = op_cf_region();
  st.splitk(p);
  if (st.status) return st.status;
  const int r = launch_igemm(p, dtype, st.s);
  if (r || rows_f32) return r;
  return st.rows_out(op, out, (size_t)M * N);
}

// softmax(scale * s, dim=-1) of fp32 rows s [rows][n] into the compute dtype (the P operand of O = P V); scale > 0, n % 4 == 0
int ldmseg_op_softmax_rows(const float* sc, int rows, int n, float scale, int dtype, float* out, void* stream) {
  if (!sc || !out || rows < 1 || n < 1 || !(scale > 0.f) || (dtype != DT_F32 && dtype != DT_BF16)) return -2;
  Stage st(stream, dtype);
  void* pp = st.buf((size_t)rows * n * esize(dtype));
  if (st.status) return st.status;
  const int r = launch_softmax_rows(sc, pp, rows, n, scale, dtype, st.s);
  if (r) return r;
  return st.rows_out(pp, out, (size_t)rows * n);
}

// argmax over C and the max-softmax probability of F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=False): x NCHW f32
// [B,C,H,W] -> ids [B,2H,2W] int64 (ignore_label where prob < mask_th, if mask_th >= 0), prob [B,2H,2W] f32 or NULL
int ldmseg_op_bilinear2x_argmax(const float* x, int B, int C, int H, int W, float mask_th, int64_t ignore_label, int dtype, int64_t* ids,
                                float* prob, void* stream) {
  if (!x || !ids || B < 1 || C < 1 || H < 1 || W < 1 || (dtype != DT_F32 && dtype != DT_BF16)) return -2;
  Stage st(stream, dtype);
  void* xp = st.nchw(x, B, C, H * W, C);
  if (st.status) return st.status;
  return launch_bilinear2x_argmax(xp, ids, prob, B, H, W, C, mask_th, ignore_label, dtype, st.s);
}

// ldmseg_op_layernorm with the choice the seg-VAE decoder makes: inplace != 0 normalises the staged tensor where it lies
// (Exec::layernorm(..., inplace = true) behind each transposed conv), 0 writes a second buffer
int ldmseg_op_layernorm_io(const float* x, const float* gamma, const float* beta, int M, int C, float eps, int silu, int inplace, int dtype,
                           float* out, void* stream) {
  if (!x || !out || M < 1 || C < 1 || (dtype != DT_F32 && dtype != DT_BF16)) return -2;
  Stage st(stream, dtype);
  void* xp = st.rows(x, (size_t)M * C);
  void* op = inplace ? xp : st.buf((size_t)M * C * esize(dtype));
  if (st.status) return st.status;
  const int r = launch_layernorm(xp, op, gamma, beta, M, C, eps, silu, dtype, st.s);
  if (r) return r;
  return st.rows_out(op, out, (size_t)M * C);
}

// F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=False): NCHW f32 in/out
int ldmseg_op_bilinear2x(const float* x, int B, int C, int H, int W, int dtype, float* out, void* stream) {
  if (B < 1 || C < 1 || H < 1 || W < 1) return -2;
  Stage st(stream, dtype);
  void* xp = st.nchw(x, B, C, H * W, C);
  if (st.status) return st.status;
  return launch_bilinear2x_nchw(xp, out, B, H, W, C, dtype, st.s);
}

int ldmseg_op_igemm(const float* x, const float* x2, const float* w, const float* bias, const float* resid,
                    const float* rowbias, int B, int Ci, int Ci2, int H, int W, int Co, int k, int stride, int up, int geglu,
                    int silu, int splits, int dtype, float* out, void* stream) {
  return op_igemm_impl(x, x2, w, bias, resid, rowbias, B, Ci, Ci2, H, W, Co, k, stride, up, geglu, silu, splits, dtype, out,
                       stream, 0, nullptr);
}
// same launch, then `iters` more back to back with HIP events around them: average microseconds per launch (incl. the
// split-K finish kernel when the plan has one).  Tuning tool (tools/kbench.py), not a product call.
int ldmseg_bench_igemm(const float* x, const float* x2, const float* w, const float* bias, const float* resid,
                       const float* rowbias, int B, int Ci, int Ci2, int H, int W, int Co, int k, int stride, int up, int geglu,
                       int silu, int splits, int dtype, int iters, float* us_per_launch, void* stream) {
  return op_igemm_impl(x, x2, w, bias, resid, rowbias, B, Ci, Ci2, H, W, Co, k, stride, up, geglu, silu, splits, dtype, nullptr,
                       stream, iters, us_per_launch);
}
int ldmseg_bench_attention(const float* qkv, int B, int N, int C, int heads, int dtype, int iters, float* us_per_launch,
                           void* stream) {
  Stage st(stream, dtype);
  hipStream_t s = st.s;
  void* qp = st.rows(qkv, (size_t)B * N * 3 * C);
  void* op = st.buf((size_t)B * N * C * esize(dtype));
  if (st.status) return st.status;
  int err = 0;
  *us_per_launch = time_launches(s, 3, iters, [&](int) { if (const int r = launch_attention(qp, op, B, N, C, heads, dtype, s)) err = err ? err : r; });
  return err;
}

// conv2d(h, w2, b2, padding=1) + conv2d(cat([xs, xs2], 1), ws, bs) - the tail of a diffusers ResnetBlock2D with a conv_shortcut -
// as the engine runs it in bf16: ONE implicit-GEMM launch whose K range continues past the nine taps with the shortcut's input
// channels read at the output pixel (IgemmParams::src2 / src3).  xs2 may be NULL (Cs2 = 0).  iters > 0: timing like
// ldmseg_bench_igemm (average microseconds per launch incl. the split-K finish).  Returns -4 when the shape has no such launch.
int ldmseg_op_conv3x3_plus_1x1(const float* h, const float* w2, const float* b2, const float* xs, const float* xs2, const float* ws,
                               const float* bs, int B, int C, int Cs, int Cs2, int H, int W, int Co, int splits, int dtype, float* out,
                               int iters, float* us_per_launch, void* stream) {
  Stage st(stream, dtype);
  hipStream_t s = st.s;
  if (dtype != DT_BF16 || C % 64 || Cs % 64 || Cs2 % 64 || !h || !w2 || !xs || !ws) return -2;
  const int HW = H * W, cs = Cs + Cs2;
  const Packed k3 = pack_weights(st, w2, b2, Co, C, 0, 3, EPI_STORE, 0, false);
  const Packed k1 = pack_weights(st, ws, bs, Co, cs, 0, 1, EPI_STORE, 0, false);
  const int Np = k3.Np;
  void* wx = st.buf((size_t)Np * (9 * C + cs) * 2);
  float* bx = (float*)st.buf(Np * sizeof(float));
  st.step([&] { return launch_concat_rows(k3.w, 9 * C, k1.w, cs, wx, Np, dtype, s) || launch_vec_add(k3.bias, k1.bias, bx, Np, s); });
  void* op = st.buf((size_t)B * HW * Co * 2);
  IgemmParams p;
  p.src0 = st.nchw(h, B, C, HW, C); p.C0 = C; p.src2 = st.nchw(xs, B, Cs, HW, Cs); p.C2 = Cs;
  p.src3 = Cs2 ? st.nchw(xs2, B, Cs2, HW, Cs2) : nullptr; p.C3 = Cs2;
  p.B = B; p.Hi = p.Ho = H; p.Wi = p.Wo = W; p.taps = 9; p.stride = 1;
  p.M = B * HW; p.N = Np; p.n_valid = Co; p.W = wx; p.bias = bx; p.out = op; p.ldo = Co; p.epi = EPI_STORE;
  if (st.status) return st.status;
  if (!igemm_xt_ok(p, dtype)) return -4;
  p.cf_ctr = op_cf_region();
  st.splitk(p, splits);
  if (st.status) return st.status;
  const int r = launch_igemm(p, dtype, s);
  if (r) return r;
  if (iters > 0 && us_per_launch) *us_per_launch = time_launches(s, 0, iters, [&](int) { (void)launch_igemm(p, dtype, s); });
  if (!out) return 0;
  return st.nchw_out(op, out, B, Co, HW, Co);
}

// the dispatch string of a described launch (igemm_plan: the chooser under the current knobs; no device)
int ldmseg_op_igemm_plan(const int* desc, int dtype, int cus, char* buf, int n) {
  if (!desc || !buf || n < 1 || cus < 1 || dtype < 0 || dtype > 3) return -2;
  IgemmLaunchDesc q;
  static_assert(sizeof q == 17 * sizeof(int), "ldmseg_op_igemm_plan takes the fields of IgemmLaunchDesc in order");
  std::memcpy(&q, desc, sizeof q);
  if (dtype >= 2) { q.x3 = dtype - 1; dtype = DT_F32; }
  IgemmDispatch d;
  if (const int r = igemm_plan(q, dtype, cus, &d)) return r;
  std::snprintf(buf, (size_t)n, "%s", igemm_dispatch_line(d).c_str());
  return 0;
}

// q[i] = n[i] / d through the multiply-shift divisor the kernels use (FastDiv, kernels.h): exactness test hook
int ldmseg_op_fastdiv(const int* n, int count, int d, int* q, void* stream) {
  if (!n || !q || count < 0 || d < 1) return -2;
  const FastDiv f = fastdiv_make(d);
  hipLaunchKernelGGL(fastdiv_probe_kernel, dim3((count + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, count, f, q);
  return launch_status();
}

// the nearest-resize source index of the loss-weight mask (nearest_index.h), evaluated on the host: CPU-suite test hook
int ldmseg_op_nearest_index(int in_size, int out_size, int* src) {
  if (!src || in_size < 1 || out_size < 1) return -2;
  for (int i = 0; i < out_size; ++i) src[i] = nearest_src_index(i, in_size, out_size);
  return 0;
}

int ldmseg_op_ln_linear(const float* x, const float* gamma, const float* beta, const float* w, const float* bias, int M, int K,
                        int N, float eps, int geglu, int dtype, float* out, void* stream) {
  return op_ln_linear_impl(x, gamma, beta, w, bias, M, K, N, eps, geglu, 0, dtype, out, stream);
}
// silu(F.linear(F.layer_norm(x), w, bias)): layer_norm2 -> mlp.fc1 of the CLIP vision executor (the 1.702 of quick_gelu is the
// caller's: it passes 1.702 w, 1.702 bias)
int ldmseg_op_ln_linear_silu(const float* x, const float* gamma, const float* beta, const float* w, const float* bias, int M,
                             int K, int N, float eps, int dtype, float* out, void* stream) {
  return op_ln_linear_impl(x, gamma, beta, w, bias, M, K, N, eps, 0, 1, dtype, out, stream);
}
// the front kernel of the CLIP vision executor (clip_vision.hip): out [B * (S/P)^2][Kpad] fp32, Kpad = 3 P P rounded up to 64
int ldmseg_op_clip_patch_rows(const float* img, int B, int H, int W, int S, int P, const float* mean, const float* std,
                              int resample, int dtype, float* out, void* stream) {
  if (B < 1 || P < 1 || S < P || S % P) return -2;
  Stage st(stream, dtype);
  const int Kpad = (int)rup(3 * P * P, 64), G = S / P;
  const size_t n = (size_t)B * G * G * Kpad;
  void* rows = st.buf(n * esize(dtype));
  if (st.status) return st.status;
  const int r = launch_clip_patch_rows(img, rows, B, H, W, S, P, Kpad, mean, std, resample, dtype, st.s);
  if (r) return r;
  return st.rows_out(rows, out, n);
}

// The tail of a transformer block on [M, C] token rows (diffusers BasicTransformerBlock + Transformer2DModel.proj_out,
// /root/reference/ldmseg/models/unet.py:401-425):
//     h2  = h + F.linear(GEGLU(F.linear(F.layer_norm(h, (C,), gamma, beta, eps), w1, b1)), w2, b2)
//     out = F.linear(h2, wp, bp) + x
// mode 0: the unfused launches (rowstats + folded-LayerNorm GEGLU GEMM + ff.net.2 GEMM + proj_out GEMM); 1: the row-local
// fused kernel for the feed-forward (tfuse.hip) + proj_out GEMM; 3: everything in the fused kernel.  bf16, C = 320 for 1 / 3.
// time_iters > 0 also times the chosen path (us per call of the whole tail).
int ldmseg_op_transformer_ff(const float* h, const float* x, const float* gamma, const float* beta, const float* w1, const float* b1,
                             const float* w2, const float* b2, const float* wp, const float* bp, int M, int C, float eps, int dtype,
                             int mode, float* out, int time_iters, float* us_per_call, void* stream) {
  Stage st(stream, dtype);
  hipStream_t s = st.s;
  const int rows_per_image = (M % 4096 == 0) ? 4096 : 0;      // (tiles rotate their chunk sweep by the index inside a 64x64 image)
  if (C % bke(dtype) || (mode != 0 && (dtype != DT_BF16 || !mlp_fused_stream_bytes(C)))) return -2;
  const int N1 = 8 * C;
  void* hp = st.buf((size_t)M * C * esize(dtype));
  void* h0 = st.rows(h, (size_t)M * C);
  void* xp = st.rows(x, (size_t)M * C);
  void* op = st.buf((size_t)M * C * esize(dtype));
  const std::vector<int> map = geglu_row_map(4 * C);
  LnFold f;
  f.w[0] = w1; f.bias[0] = b1; f.Nper = N1; f.K = C; f.Npad = N1; f.gamma = gamma; f.beta = beta; f.row_map = &map; f.dtype = dtype;
  void* w1p = st.buf((size_t)N1 * C * esize(dtype));
  float* c1 = (float*)st.buf(N1 * sizeof(float));
  float* c2 = (float*)st.buf(N1 * sizeof(float));
  void* scratch = st.buf(ln_fold_scratch_bytes(f));
  st.step([&] { return launch_ln_fold(f, scratch, w1p, c1, c2, s); });
  void* w2p = st.rows(w2, (size_t)C * 4 * C);        // Linear weights are already [N][K]
  void* wpp = st.rows(wp, (size_t)C * C);
  float* b2d = st.floats(b2, C);
  float* bpd = st.floats(bp, C);
  void* stream_w = nullptr;
  if (mode != 0) {
    stream_w = st.buf(mlp_fused_stream_bytes(C));
    st.step([&] { return launch_pack_mlp_stream(w1p, w2p, wpp, stream_w, C, s); });
  }
  float* stats = (float*)st.buf((size_t)M * 2 * sizeof(float));
  void* ff = st.buf((size_t)M * 4 * C * esize(dtype));
  st.step([&] { return igemm_warm(); });
  if (st.status) return st.status;
  auto gemm = [&](const void* src, int K, const void* W, int N, int nvalid, const float* bias, const void* resid, void* o, int epi,
                  const float* rs, const float* cc1) -> int {
    IgemmParams p;
    p.src0 = src; p.C0 = K; p.B = 1; p.Hi = p.Ho = M; p.Wi = p.Wo = 1;
    p.M = M; p.N = N; p.n_valid = nvalid; p.W = W; p.bias = bias; p.rowstats = rs; p.c1 = cc1;
    p.resid = resid; p.ldr = C; p.out = o; p.ldo = nvalid; p.epi = epi;
    st.splitk(p);
    return st.status ? st.status : launch_igemm(p, dtype, s);
  };
  auto run = [&]() -> int {
    (void)hipMemcpyAsync(hp, h0, (size_t)M * C * esize(dtype), hipMemcpyDeviceToDevice, s);   // the tail updates h in place
    if (mode == 0) {
      if (int r = launch_rowstats(hp, stats, M, C, eps, dtype, s)) return r;
      if (int r = gemm(hp, C, w1p, N1, 4 * C, c2, nullptr, ff, EPI_GEGLU, stats, c1)) return r;
      if (int r = gemm(ff, 4 * C, w2p, C, C, b2d, hp, hp, EPI_STORE, nullptr, nullptr)) return r;
      return gemm(hp, C, wpp, C, C, bpd, xp, op, EPI_STORE, nullptr, nullptr);
    }
    const int proj = (mode & 2) ? 1 : 0;
    if (int r = launch_mlp_fused(hp, proj ? op : hp, xp, stream_w, c2, b2d, bpd, igemm_zero_page(), M, C, eps, proj, rows_per_image, s)) return r;
    return proj ? 0 : gemm(hp, C, wpp, C, C, bpd, xp, op, EPI_STORE, nullptr, nullptr);
  };
  if (int r = run()) return r;
  if (time_iters > 0 && us_per_call) *us_per_call = time_launches(s, 2, time_iters, [&](int) { (void)run(); });
  return st.rows_out(op, out, (size_t)M * C);
}

int ldmseg_op_transformer_in(const float* x, const float* wp, const float* bp, const float* gamma, const float* beta, const float* wq,
                             const float* wk, const float* wv, int M, int C, float eps, int dtype, int mode, float* h_out, float* qkv_out,
                             int time_iters, float* us_per_call, void* stream) {
  return transformer_in_impl(x, nullptr, nullptr, 0.f, 0, 0, wp, bp, gamma, beta, wq, wk, wv, M, C, eps, dtype, mode, h_out, qkv_out,
                             time_iters, us_per_call, stream);
}
// The same behind the transformer's GroupNorm (32 groups, no SiLU) over x = [images][M / images][C] rows: gn_mode 0 = a GroupNorm
// launch, then the entry as above; gn_mode 1 (mode 1 only) = statistics pass + the apply sweep inside the fused kernel (tproj.hip).
int ldmseg_op_gn_transformer_in(const float* x, const float* gn_gamma, const float* gn_beta, float gn_eps, int images, int gn_mode,
                                const float* wp, const float* bp, const float* gamma, const float* beta, const float* wq,
                                const float* wk, const float* wv, int M, int C, float eps, int dtype, int mode, float* h_out,
                                float* qkv_out, int time_iters, float* us_per_call, void* stream) {
  if (!gn_gamma || !gn_beta) return -2;
  return transformer_in_impl(x, gn_gamma, gn_beta, gn_eps, images, gn_mode, wp, bp, gamma, beta, wq, wk, wv, M, C, eps, dtype, mode, h_out,
                             qkv_out, time_iters, us_per_call, stream);
}

// The step tail kernel (tail.hip, bf16): eps = conv2d(x, w, bias, padding=1) with 320 -> 4 channels on [B,320,H,W] and, when
// ddim != 0, the scheduler update of `latents` (in place; last != 0: pred_original_sample), the inpainting paste, the
// self-condition write and the next step's packed input (returned as fp32 [B, H*W, 64]).  eps_out / cond / xin_out / known
// may be null.  coef4 = {sqrt_alpha_t, sqrt_beta_t, sqrt_alpha_prev, sqrt_beta_prev} (host).
int ldmseg_op_conv_out_tail(const float* x, const float* w, const float* bias, int B, int H, int W, float* eps_out, int ddim, int last,
                            const float* coef4, int pred_type, int clip, float clip_range, float* latents, float* cond,
                            const float* rgb, const uint8_t* known, const float* z0, const float* noise, float sa, float sb,
                            float* xin_out, void* stream) {
  Stage st(stream, DT_BF16);
  hipStream_t s = st.s;
  if (!conv_out_tail_ok(320, H, W, DT_BF16) || (ddim && (!coef4 || !latents))) return -2;
  const Packed wk = pack_weights(st, w, bias, 4, 320, 0, 3, EPI_STORE, 0, false);
  st.step([&] { return igemm_warm(); });
  StepTail t;
  t.x = st.nchw(x, B, 320, H * W, 320); t.w = wk.w; t.bias = wk.bias; t.zeros = igemm_zero_page(); t.B = B; t.H = H; t.W = W; t.eps_out = eps_out;
  void* xin = nullptr;
  if (ddim) {
    t.ddim = 1; t.last = last;
    t.c = DdimCoef{coef4[0], coef4[1], coef4[2], coef4[3], pred_type, clip, clip_range, 0};
    t.latents = latents; t.cond = cond; t.rgb = rgb; t.known = known; t.z0 = z0; t.noise = noise; t.sa = sa; t.sb = sb;
    if (xin_out) {
      xin = st.buf((size_t)B * H * W * 64 * 2);
      st.step([&] { return hipMemsetAsync(xin, 0xff, (size_t)B * H * W * 64 * 2, s) != hipSuccess; });
      t.xin_next = xin;
    }
  }
  if (st.status) return st.status;
  const int r = launch_conv_out_tail(t, s);
  if (r) return r;
  if (xin && !last) return st.rows_out(xin, xin_out, (size_t)B * H * W * 64);
  return 0;
}

// the same attention on the fp8 (e4m3) operand path of the bf16 mode (attention_fp8.hip): head dim 40 or 80
int ldmseg_op_attention_fp8(const float* qkv, int B, int N, int C, int heads, float* out, int time_iters, float* us_per_launch,
                            void* stream) {
  Stage st(stream, DT_BF16);
  hipStream_t s = st.s;
  const size_t kv = attention_fp8_scratch_bytes(B, N, C, heads);
  if (!kv) return -2;
  void* qp = st.rows(qkv, (size_t)B * N * 3 * C);
  void* op = st.buf((size_t)B * N * C * 2);
  void* kp = st.buf(kv);
  if (st.status) return st.status;
  int r = launch_attention_fp8(qp, kp, op, B, N, C, heads, s);
  if (r) return r;
  if (time_iters > 0 && us_per_launch) {
    *us_per_launch = time_launches(s, 2, time_iters, [&](int) { (void)launch_attention_fp8(qp, kp, op, B, N, C, heads, s); });
  }
  if (out) return st.rows_out(op, out, (size_t)B * N * C);
  return 0;
}

// ------------------------------------------------------------------ the seg-VAE decoder's backward kernels (vae_bwd.hip), fp32 tensors
// dtype: 0 = fp32 products, 2 / 3 = split-bf16 products (3: data-gradient weights as hi | lo planes, as a bf16x3 handle holds them)
// rows (image, Y, X) of a [B, 2H * 2W, C] map -> phase-major [B, H, W, 2x2, C] (what launch_ln_silu_bwd stores with pm = 1)
static __global__ void phase_major_rows_kernel(const float* x, float* y, int H2, int W2, int C, size_t total) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(e % C);
    const size_t r = e / C;
    y[phase_major_row(r, H2, W2) * C + c] = x[e];
  }
}
static float* stage_phase_major(Stage& st, const float* dy, int B, int Co, int H, int W) {
  const size_t total = (size_t)B * 4 * H * W * Co;
  float* rows = (float*)st.nchw(dy, B, Co, 4 * H * W, Co);
  float* pm = (float*)st.buf(total * sizeof(float));
  st.step([&] {
    hipLaunchKernelGGL(phase_major_rows_kernel, dim3(rows_grid(total)), dim3(256), 0, st.s, rows, pm, 2 * H, 2 * W, Co, total);
    return hipGetLastError() != hipSuccess;
  });
  return st.status ? nullptr : pm;
}
static int op_wgrad_run(Stage& st, WgradParams& wp, int form, int n_real, int c_real, int co, float* dw) {
  WgradPlan pl;
  if (wgrad_plan(wp, wgrad_cus(), &pl)) return -2;
  wp.partial = (float*)st.buf(wgrad_partial_bytes(wp, pl));
  if (st.status) return st.status;
  return launch_wgrad(wp, pl, {form, n_real, c_real, co, dw}, st.s);
}
// the bias gradient that follows a weight gradient: db[j] = the sum over the P rows of dy [P][lda] and q < Q of column q * qstride + j
static int op_bias_colsum(Stage& st, const float* dy, int lda, int P, int Q, int qstride, int n, float* db) {
  float* scratch = (float*)st.buf(colsum_scratch_bytes(P, lda));
  if (st.status) return st.status;
  return launch_colsum(dy, lda, P, lda, Q, qstride, n, scratch, db, st.s);
}
// grads of F.conv2d(x, w, b, stride=stride, padding=1) with respect to w and b (arguments checked by the entries)
static int op_conv_wgrad(const float* x, const float* dy, int B, int Ci, int H, int W, int Co, int stride, WgradRule rule, int dtype, float* dw,
                         float* db, void* stream) {
  Stage st(stream, dtype, true);
  const int Ho = conv_out_dim(H, stride), Wo = conv_out_dim(W, stride);
  const int Cip = (int)rup(Ci, 32), Cop = (int)rup(Co, 32), P = B * Ho * Wo;
  WgradParams wp;
  wp.x = (const float*)st.nchw(x, B, Ci, H * W, Cip); wp.C = Cip;
  wp.dy = (const float*)st.nchw(dy, B, Co, Ho * Wo, Cop); wp.ldy = Cop; wp.N = Cop;
  wp.B = B; wp.H = H; wp.W = W; wp.taps = 9; wp.x3 = st.x3 ? 1 : 0; wp.stride = stride; wp.rule = rule;
  const int r = op_wgrad_run(st, wp, 0, Co, Ci, 0, dw);
  if (r || !db) return r;
  return op_bias_colsum(st, wp.dy, Cop, P, 1, 0, Co, db);
}

// grads of F.conv2d(x, w, b, padding=1) with respect to w and b: x [B,Ci,H,W], dy [B,Co,H,W] -> dw [Co,Ci,3,3], db [Co] or NULL
int ldmseg_op_conv_wgrad(const float* x, const float* dy, int B, int Ci, int H, int W, int Co, int dtype, float* dw, float* db, void* stream) {
  if (!x || !dy || !dw || B < 1 || Ci < 1 || Co < 1 || H < 1 || W < 1 || (dtype != 0 && dtype != 2 && dtype != 3)) return -2;
  return op_conv_wgrad(x, dy, B, Ci, H, W, Co, 1, kWgradFixedTile, dtype, dw, db, stream);
}
// grads of F.conv_transpose2d(x, w, b, stride=2) (kernel 2): x [B,Ci,H,W], dy [B,Co,2H,2W] -> dw [Ci,Co,2,2], db [Co] or NULL
int ldmseg_op_convt2_wgrad(const float* x, const float* dy, int B, int Ci, int H, int W, int Co, int dtype, float* dw, float* db, void* stream) {
  if (!x || !dy || !dw || B < 1 || Ci < 1 || Co < 4 || Co % 4 || H < 1 || W < 1 || (dtype != 0 && dtype != 2 && dtype != 3)) return -2;
  Stage st(stream, dtype, true);
  const int Cip = (int)rup(Ci, 32), P = B * H * W;
  WgradParams wp;
  wp.x = (const float*)st.nchw(x, B, Ci, H * W, Cip); wp.C = Cip;
  wp.dy = stage_phase_major(st, dy, B, Co, H, W); wp.ldy = 4 * Co; wp.N = 4 * Co;
  wp.B = B; wp.H = H; wp.W = W; wp.taps = 1; wp.x3 = st.x3 ? 1 : 0;
  const int r = op_wgrad_run(st, wp, 1, 4 * Co, Ci, Co, dw);
  if (r || !db) return r;
  return op_bias_colsum(st, wp.dy, 4 * Co, P, 4, Co, Co, db);
}
// grad of F.conv2d(x, w, padding=1) with respect to x, the way ldmseg_vae_decode_backward runs it: igemm on the transposed, rotated
// packing.  dy [B,Co,H,W], w [Co,Ci,3,3] -> dx [B,Ci,H,W]; nchw_epi: the fp32 NCHW store epilogue (the latents' gradient)
int ldmseg_op_conv_dgrad(const float* dy, const float* w, int B, int Ci, int H, int W, int Co, int nchw_epi, int dtype, float* dx, void* stream) {
  if (!dy || !w || !dx || B < 1 || Ci < 1 || Co < 1 || H < 1 || W < 1 || (dtype != 0 && dtype != 2 && dtype != 3)) return -2;
  if (!nchw_epi && Ci % 4) return -2;
  Stage st(stream, dtype, true);
  hipStream_t s = st.s;
  const int epi = nchw_epi ? EPI_NCHW_F32 : EPI_STORE;
  const DgradShape ds = dgrad_conv_shape(Co, Ci, epi);
  const int Cop = ds.cin_pad, Np = ds.N, P = B * H * W;
  float* wp = (float*)st.buf((size_t)Np * 9 * Cop * sizeof(float));
  st.step([&] { return launch_pack_dgrad_conv(w, wp, Co, Ci, Np, Cop, s) || (st.x3 == 2 && launch_split_planes(wp, (size_t)Np * 9 * Cop, s)); });
  IgemmParams p;
  p.src0 = st.nchw(dy, B, Co, H * W, Cop); p.C0 = Cop; p.B = B; p.Hi = p.Ho = H; p.Wi = p.Wo = W;
  p.taps = 9; p.M = P; p.N = Np; p.n_valid = Ci; p.W = wp; p.epi = epi; p.x3 = st.x3;
  void* op = nchw_epi ? (void*)dx : st.buf((size_t)P * Ci * sizeof(float));
  p.out = op; p.ldo = Ci;
  p.cf_ctr = op_cf_region();
  st.splitk(p);
  if (st.status) return st.status;
  const int r = launch_igemm(p, DT_F32, s);
  if (r || nchw_epi) return r;
  return st.nchw_out(op, dx, B, Ci, H * W, Ci);
}
// grad of F.conv_transpose2d(x, w, stride=2) (kernel 2) with respect to x: dy [B,Co,2H,2W], w [Ci,Co,2,2] -> dx [B,Ci,H,W]
int ldmseg_op_convt2_dgrad(const float* dy, const float* w, int B, int Ci, int H, int W, int Co, int dtype, float* dx, void* stream) {
  if (!dy || !w || !dx || B < 1 || Ci < 4 || Ci % 4 || Co < 8 || Co % 8 || H < 1 || W < 1 || (dtype != 0 && dtype != 2 && dtype != 3)) return -2;
  Stage st(stream, dtype, true);
  hipStream_t s = st.s;
  const int Np = dgrad_convt_shape(Ci, Co).N, P = B * H * W;
  float* wp = (float*)st.buf((size_t)Np * 4 * Co * sizeof(float));
  st.step([&] { return launch_pack_dgrad_convt(w, wp, Ci, Co, Np, s) || (st.x3 == 2 && launch_split_planes(wp, (size_t)Np * 4 * Co, s)); });
  IgemmParams p;
  p.src0 = stage_phase_major(st, dy, B, Co, H, W); p.C0 = 4 * Co; p.B = B; p.Hi = p.Ho = H; p.Wi = p.Wo = W;
  p.taps = 1; p.M = P; p.N = Np; p.n_valid = Ci; p.W = wp; p.epi = EPI_STORE; p.x3 = st.x3;
  void* op = st.buf((size_t)P * Ci * sizeof(float));
  p.out = op; p.ldo = Ci;
  p.cf_ctr = op_cf_region();
  st.splitk(p);
  if (st.status) return st.status;
  const int r = launch_igemm(p, DT_F32, s);
  if (r) return r;
  return st.nchw_out(op, dx, B, Ci, H * W, Ci);
}
// backward of F.silu(F.group_norm(x, 32, gamma, beta, eps)): x, dy [B,C,HW] -> dx [B,C,HW], dgamma / dbeta [C] or NULL
int ldmseg_op_groupnorm_silu_bwd(const float* x, const float* dy, const float* gamma, const float* beta, int B, int C, int HW, float eps,
                                 float* dx, float* dgamma, float* dbeta, void* stream) {
  if (!x || !dy || !gamma || !beta || !dx || B < 1 || C < 32 || C % 32 || HW < 1) return -2;
  Stage st(stream, DT_F32);
  const float* xp = (const float*)st.nchw(x, B, C, HW, C);
  const float* dp = (const float*)st.nchw(dy, B, C, HW, C);
  float* op = (float*)st.buf((size_t)B * HW * C * sizeof(float));
  float* scratch = (float*)st.buf(gn_bwd_scratch_bytes(B, C));
  if (st.status) return st.status;
  const int r = launch_gn_silu_bwd(xp, dp, gamma, beta, op, dgamma, dbeta, B, HW, C, eps, scratch, st.s);
  if (r) return r;
  return st.nchw_out(op, dx, B, C, HW, C);
}
// backward of F.silu(F.layer_norm(x, (C,), gamma, beta, eps)) over rows: x, dy [M,C] -> dx [M,C], dgamma / dbeta [C] or NULL.
// pm = 1: the rows are the pixels of maps H2 x W2 and dx is stored phase-major, [image][H2/2][W2/2][2x2][C].
int ldmseg_op_layernorm_silu_bwd(const float* x, const float* dy, const float* gamma, const float* beta, int M, int C, float eps, int pm,
                                 int H2, int W2, float* dx, float* dgamma, float* dbeta, void* stream) {
  if (!x || !dy || !gamma || !beta || !dx || M < 1 || C < 64 || C % 64 || C > 1024) return -2;
  if (pm && (H2 < 2 || W2 < 2 || (H2 & 1) || (W2 & 1) || M % (H2 * W2))) return -2;
  Stage st(stream, DT_F32);
  float* scratch = (float*)st.buf(ln_bwd_scratch_bytes(M, C));
  if (st.status) return st.status;
  return launch_ln_silu_bwd(x, dy, gamma, beta, dx, dgamma, dbeta, M, C, eps, pm, H2, W2, scratch, st.s);
}
// The plan of a weight-gradient launch (wgrad_plan.h; no device): P pixels, N columns of dY, C storage channels of X, taps 9 | 1,
// x3 0 | 1, on a device of `cus` CUs.  buf receives wgrad_plan_line; -2 where there is no such launch.
int ldmseg_op_wgrad_plan(int P, int N, int C, int taps, int x3, int cus, char* buf, int n) {
  if (!buf || n < 1) return -2;
  WgradPlan pl;
  const int r = wgrad_choose(WgradDesc{P, N, C, taps, x3}, kWgradFixedTile, cus, &pl);
  if (r == 0) std::snprintf(buf, (size_t)n, "%s", wgrad_plan_line(pl).c_str());
  return r;
}

// ------------------------------------------------------------------ what the encoder's backward adds
// grads of F.conv2d(x, w, b, stride=stride, padding=1) with respect to w and b on the by-width tile: x [B,Ci,H,W], dy [B,Co,Ho,Wo]
int ldmseg_op_conv_wgrad_ex(const float* x, const float* dy, int B, int Ci, int H, int W, int Co, int stride, int dtype, float* dw, float* db,
                            void* stream) {
  if (!x || !dy || !dw || B < 1 || Ci < 1 || Co < 1 || H < 1 || W < 1 || (stride != 1 && stride != 2) || (dtype != 0 && dtype != 2 && dtype != 3))
    return -2;
  return op_conv_wgrad(x, dy, B, Ci, H, W, Co, stride, kWgradByWidth, dtype, dw, db, stream);
}
int ldmseg_op_conv_s2_wgrad(const float* x, const float* dy, int B, int Ci, int H, int W, int Co, int dtype, float* dw, float* db, void* stream) {
  return ldmseg_op_conv_wgrad_ex(x, dy, B, Ci, H, W, Co, 2, dtype, dw, db, stream);
}
// NHWC [B][H2][W2][C] -> the top-left H x W of every map as NCHW [B][C][H][W] (an odd map's data gradient: the scatter fills 2 Ho x 2 Wo)
static __global__ void crop_nhwc_kernel(const float* x, float* y, int C, int H, int W, int H2, int W2, size_t total) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int xx = (int)(e % W), yy = (int)((e / W) % H), c = (int)((e / ((size_t)W * H)) % C);
    const size_t b = e / ((size_t)W * H * C);
    y[e] = x[((b * H2 + yy) * W2 + xx) * C + c];
  }
}
// grad of F.conv2d(x, w, stride=2, padding=1) with respect to x, the way ldmseg_vae_encode_backward runs it: one igemm launch over
// dY [B,Co,Ho,Wo] (3x3 window, pad 1) on the phase packing, N = 4 Ci, scattered to the 2 Ho x 2 Wo map by EPI_CONVT2
int ldmseg_op_conv_s2_dgrad(const float* dy, const float* w, int B, int Ci, int H, int W, int Co, int dtype, float* dx, void* stream) {
  if (!dy || !w || !dx || B < 1 || Ci < 4 || Ci % 4 || Co < 1 || H < 1 || W < 1 || (dtype != 0 && dtype != 2 && dtype != 3)) return -2;
  Stage st(stream, dtype, true);
  hipStream_t s = st.s;
  const int Ho = conv_out_dim(H, 2), Wo = conv_out_dim(W, 2);
  const DgradShape ds = dgrad_conv_s2_shape(Co, Ci);
  const int Cop = ds.cin_pad, Np = ds.N, P = B * Ho * Wo;
  float* wp = (float*)st.buf((size_t)Np * 9 * Cop * sizeof(float));
  st.step([&] { return launch_pack_dgrad_conv_s2(w, wp, Co, Ci, Np, Cop, s) || (st.x3 == 2 && launch_split_planes(wp, (size_t)Np * 9 * Cop, s)); });
  IgemmParams p;
  p.src0 = st.nchw(dy, B, Co, Ho * Wo, Cop); p.C0 = Cop; p.B = B; p.Hi = p.Ho = Ho; p.Wi = p.Wo = Wo;
  p.taps = 9; p.M = P; p.N = Np; p.n_valid = 4 * Ci; p.W = wp; p.epi = EPI_CONVT2; p.cout = Ci; p.x3 = st.x3;
  float* op = (float*)st.buf((size_t)4 * P * Ci * sizeof(float));
  p.out = op; p.ldo = Ci;
  p.cf_ctr = op_cf_region();
  if (st.status) return st.status;
  const int r = launch_igemm(p, DT_F32, s);
  if (r) return r;
  if (H == 2 * Ho && W == 2 * Wo) return st.nchw_out(op, dx, B, Ci, H * W, Ci);
  const size_t total = (size_t)B * Ci * H * W;
  hipLaunchKernelGGL(crop_nhwc_kernel, dim3(rows_grid(total)), dim3(256), 0, s, op, dx, Ci, H, W, 2 * Ho, 2 * Wo, total);
  return launch_status();
}
int ldmseg_op_silu_bwd(const float* u, const float* da, int64_t n, float* du, void* stream) {
  if (!u || !da || !du || n < 1) return -2;
  return launch_silu_bwd(u, da, du, (size_t)n, (hipStream_t)stream);
}
// a = silu(u): the launch that follows a SiLU-less conv inside the encoder's backward
int ldmseg_op_silu_fwd(const float* u, int64_t n, float* a, void* stream) {
  if (!u || !a || n < 1) return -2;
  return launch_silu_fwd(u, a, (size_t)n, (hipStream_t)stream);
}
// ldmseg_op_wgrad_plan of the by-width rule (kWgradByWidth): P = the pixels of the OUTPUT map of a conv of stride 1 | 2
int ldmseg_op_wgrad_plan_ex(int P, int N, int C, int taps, int x3, int stride, int cus, char* buf, int n, int64_t* macs_per_pixel) {
  if (!buf || n < 1) return -2;
  WgradPlan pl;
  const int r = wgrad_choose(WgradDesc{P, N, C, taps, x3, stride}, kWgradByWidth, cus, &pl);
  if (r == 0) {
    std::snprintf(buf, (size_t)n, "%s", wgrad_plan_line(pl).c_str());
    if (macs_per_pixel) *macs_per_pixel = wgrad_plan_macs_per_pixel(pl);
  }
  return r;
}

// The two fp32 kernels of the time embedding (misc.hip) on the caller's device tensors: nothing is staged or converted.
// _time_sinusoid: out [B][320] = [cos(t f_i) | sin(t f_i)] of t_dev (int64, t_count = 1 broadcasts, t_count = B per row) or, NULL, t_host.
int ldmseg_op_time_sinusoid(const int64_t* t_dev, int t_count, int64_t t_host, int B, float* out, void* stream) {
  if (B < 1 || !out || (t_dev && t_count != 1 && t_count != B)) return -2;
  return launch_time_embed(t_dev, t_count, t_host, B, out, (hipStream_t)stream);
}
// _small_linear: y [B][N] = act_out(act_in(x [B][K]) W[N][K]^T + bias [N] or NULL), act = SiLU where its flag is set; any B >= 1.
int ldmseg_op_small_linear(const float* x, const float* W, const float* bias, int B, int K, int N, int silu_in, int silu_out, float* y,
                           void* stream) {
  if (!x || !W || !y || B < 1 || K < 1 || N < 1) return -2;
  return launch_small_linear(x, W, bias, y, B, K, N, silu_in, silu_out, (hipStream_t)stream);
}

}  // extern "C"
