// Host runtime of libldmseg_hip.so, the part every model file (unet.hip, vae.hip, clip.hip) shares: error reporting, the
// profiler, device memory, weight repacking (Builder), workspace planning and the executor (Exec) that turns layers into
// launches.  The single definitions behind the declarations here are in runtime.hip.
//
// Layout in HBM: activations NHWC [B, H*W, C] in the compute dtype; conv/linear weights [N][K] with
// K = (tap, channel) so one 128-B line of a weight row is one K tile; norm parameters, biases and the time-embedding MLP
// stay fp32.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/ldmseg_hip.h"
#include "attn_plan.h"
#include "kernels.h"
#include "workspace.h"

namespace ldmseg::rt {

extern thread_local std::string g_err;      // behind fail() and ldmseg_last_error()
// Bumped whenever a process-global tuning knob that the workspace plan depends on changes (debug_knobs.hip: the rows with
// `replans`, e.g. tile policy and forced instantiation decide the split-K slice counts, i.e. the size of the partial-sum
// scratch).  Handles remember the epoch their cached plan was made under and re-plan when it moved.
extern int g_plan_epoch;
extern int g_gnfold_mode;          // debug key 22
extern int g_sepenc_every_step;    // debug key 25
extern int g_ffp_mode;             // debug key 20

inline int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t e__ = (expr);                                                                  \
    if (e__ != hipSuccess)                                                                    \
      return fail(LDMSEG_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));          \
  } while (0)
#define TRY(expr)                                                                             \
  do {                                                                                        \
    int r__ = (expr);                                                                         \
    if (r__ != 0) {                                                                           \
      if (g_err.empty())                                                                      \
        g_err = std::string(#expr) + " failed (" + std::to_string(r__) + ")" +                \
                (r__ == -3 ? std::string(": ") + hipGetErrorString(hipGetLastError()) : ""); \
      return r__;                                                                             \
    }                                                                                         \
  } while (0)

// A launcher's return code (0, -2 shape, -3 a HIP error) as the ABI's, with `what` as the message.  arg_what: the -2 of this launcher
// means a bad argument of the caller (LDMSEG_E_ARG with that message).
inline int launch_code(int r, const char* what, const char* arg_what = nullptr) {
  if (r == 0) return 0;
  if (r == -2 && arg_what) return fail(LDMSEG_E_ARG, arg_what);
  return fail(r == -2 ? LDMSEG_E_SHAPE : LDMSEG_E_HIP, what + (r == -3 ? std::string(": ") + hipGetErrorString(hipGetLastError()) : std::string()));
}

// Makes `device` current for the duration of a call on a handle (a process may hold handles on several GPUs; the
// kernels, workspaces and per-device launcher state of a handle all belong to cfg.device) and restores the caller's.
struct DeviceGuard {
  int prev = -1;
  bool changed = false;
  explicit DeviceGuard(int device) {
    if (hipGetDevice(&prev) == hipSuccess && prev != device) changed = hipSetDevice(device) == hipSuccess;
  }
  ~DeviceGuard() {
    if (changed) (void)hipSetDevice(prev);
  }
};

int alloc_gn_sync(void** out);   // a handle's hand-off region of the cooperative GroupNorm kernel (norm.hip), zeroed once
int alloc_cf_sync(void** out);   // a handle's counter region of the in-launch split-K finish (igemm.hip, IgemmParams::cf_ctr), zeroed once
inline size_t esize(int dt) { return dt == DT_BF16 ? 2 : 4; }
inline int bke(int dt) { return dt == DT_BF16 ? 64 : 32; }  // channels per 128-B K tile

// ------------------------------------------------------------------ profiling
struct ProfFamily {
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
  std::vector<std::string> label;
  std::vector<double> lflops;
  int64_t launches = 0;
  double flops = 0, bytes = 0;
};
struct Profiler {
  bool on = false;
  ProfFamily fam[5];
  std::vector<hipEvent_t> pool;
  hipEvent_t get() {
    if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
  }
};
extern Profiler g_prof;

inline constexpr auto no_label = [] { return std::string(); };

// ------------------------------------------------------------------ device memory
struct DeviceArena {  // persistent parameters: chunked bump allocator
  std::vector<void*> chunks;
  char* cur = nullptr;
  size_t left = 0;
  size_t total = 0;
  int alloc(void** out, size_t bytes) {
    bytes = rup(bytes, 256);
    if (bytes > left) {
      const size_t chunk = bytes > ((size_t)256 << 20) ? bytes : ((size_t)256 << 20);
      void* p = nullptr;
      if (hipMalloc(&p, chunk) != hipSuccess) return fail(LDMSEG_E_OOM, "hipMalloc of parameter chunk failed");
      chunks.push_back(p);
      cur = (char*)p;
      left = chunk;
      total += chunk;
    }
    *out = cur;
    cur += bytes;
    left -= bytes;
    return 0;
  }
  void release() {
    for (void* p : chunks) (void)hipFree(p);
    chunks.clear();
    cur = nullptr;
    left = 0;
  }
};

struct WeightMap {
  std::unordered_map<std::string, std::pair<const float*, int64_t>> m;
  int get(const std::string& key, int64_t numel, const float** out) const {
    auto it = m.find(key);
    if (it == m.end()) return fail(LDMSEG_E_WEIGHT, "missing state-dict key: " + key);
    if (it->second.second != numel)
      return fail(LDMSEG_E_WEIGHT, "state-dict key " + key + " has " + std::to_string(it->second.second) +
                                       " elements, expected " + std::to_string(numel));
    *out = it->second.first;
    return 0;
  }
};

struct ConvW {
  void* w = nullptr;      // [N][taps*cin_pad]
  float* bias = nullptr;  // [N]
  float* c1 = nullptr;    // [N] row sums of w when a LayerNorm is folded into this GEMM (IgemmParams::c1), else null
  int N = 0, n_valid = 0, cin_pad = 0, taps = 1, cout = 0;
  void* w_cm = nullptr;   // 3x3 layers that may run on large maps: second packing in channel-major K order (IgemmParams::cm)
  void* w_up4 = nullptr;  // upsampler convs, bf16: [4 phases][N][2x2 taps][C] with the 3x3 taps pre-summed per phase (IgemmParams::up4)
  int xt_cin = 0;         // extra-tap packings (ResnetW::conv2x): input channels of the 1x1 part behind the nine taps' columns
};
struct NormW { float* g = nullptr; float* b = nullptr; int C = 0; };
// the shape of a Conv2d / Linear packing [Npad][k*k][cin_pad]: n_store >= Co forces explicit zero output channels, epi decides the N tile
inline void conv_shape(int Co, int k, int cin_pad, int n_store, int epi, ConvW* out) {
  const int nreal = n_store > Co ? n_store : Co;
  out->N = (int)rup(nreal, igemm_pick_bn(nreal, epi));
  out->n_valid = nreal;
  out->cin_pad = cin_pad;
  out->taps = k * k;
  out->cout = Co;
}

// What every handle owns: its device and compute mode, the parameter arena, the workspace with its cached plan and the two
// hand-off regions of its launches.  The four public handle types derive from it.
struct HandleBase {
  int device = 0;
  int dt = DT_BF16;
  bool x3 = false;      // fp32 storage with split-bf16 GEMM arithmetic (LDMSEG_BF16X3)
  DeviceArena arena;
  Workspace ws;
  void* ws_mem = nullptr;
  size_t ws_cap = 0;
  int64_t nparams = 0;
  void* gn_sync = nullptr;     // cooperative GroupNorm (null: a handle without GroupNorm launches)
  void* cf_sync = nullptr;     // in-launch split-K finish
  // plan_workspace: the shape key the sizes below were measured for (plan_key[4] = g_plan_epoch then)
  int plan_key[5] = {};
  bool plan_valid = false;
  size_t plan_persist = 0, plan_scratch = 0;
  ~HandleBase() {
    DeviceGuard dg(device);    // (the caller's current device may be another one)
    arena.release();
    if (ws_mem) (void)hipFree(ws_mem);
    if (gn_sync) (void)hipFree(gn_sync);
    if (cf_sync) (void)hipFree(cf_sync);
  }
};

struct Builder {      // repacks a state dict into the arena of the handle it is made for, on the null stream
  Builder(HandleBase& h, const WeightMap& w) : arena(&h.arena), wm(&w), dt(h.dt), s(nullptr), x3(h.x3) {}
  DeviceArena* arena;
  const WeightMap* wm;
  int dt;
  hipStream_t s;
  int64_t nparams = 0;
  std::vector<void*> temps;
  bool x3 = false;                                         // LDMSEG_BF16X3 handle: every GEMM weight matrix becomes hi | lo planes at finish()
  std::vector<std::pair<void*, size_t>> x3_w;              // (packed fp32 matrix, floats)
  void* fold_scratch = nullptr;                            // ln_linear
  size_t fold_cap = 0;
  void weights(void* w, size_t nfloats) { if (x3 && dt == DT_F32) x3_w.emplace_back(w, nfloats); }

  int f32_copy(const std::string& key, int64_t n, float** out) {
    const float* src;
    TRY(wm->get(key, n, &src));
    void* p;
    TRY(arena->alloc(&p, n * sizeof(float)));
    HIP_TRY(hipMemcpyAsync(p, src, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    *out = (float*)p;
    nparams += n;
    return 0;
  }
  // [Npad] bias of a GEMM: the n values of `key` (null: none), zeros behind them
  int padded_bias(const std::string* key, int n, int Npad, float** out) {
    const float* src = nullptr;
    if (key) TRY(wm->get(*key, n, &src));
    void* p;
    TRY(arena->alloc(&p, Npad * sizeof(float)));
    TRY(launch_padded_bias(src, n, (float*)p, Npad, s));
    *out = (float*)p;
    if (key) nparams += n;
    return 0;
  }
  int norm(const std::string& prefix, int C, NormW* out) {
    out->C = C;
    TRY(f32_copy(prefix + ".weight", C, &out->g));
    TRY(f32_copy(prefix + ".bias", C, &out->b));
    return 0;
  }
  // Conv2d / Linear: OIHW -> [Npad][k*k][cin_pad]; n_store >= Co forces explicit zero output channels
  int conv(const std::string& prefix, int Co, int Ci, int k, int cin_pad, ConvW* out, bool has_bias = true,
           int n_store = 0, int epi = EPI_STORE, bool cm = false) {
    const float* w;
    TRY(wm->get(prefix + ".weight", (int64_t)Co * Ci * k * k, &w));
    conv_shape(Co, k, cin_pad, n_store, epi, out);
    const int Npad = out->N;
    TRY(arena->alloc(&out->w, (size_t)Npad * k * k * cin_pad * esize(dt)));
    TRY(launch_repack_conv(w, out->w, Co, Ci, k, k, Npad, cin_pad, dt, s));
    weights(out->w, (size_t)Npad * k * k * cin_pad);
    if (cm && k == 3 && cin_pad % bke(dt) == 0 && dt == DT_BF16 && Npad % 160 == 0) {
      TRY(arena->alloc(&out->w_cm, (size_t)Npad * k * k * cin_pad * esize(dt)));
      TRY(launch_repack_conv(w, out->w_cm, Co, Ci, k, k, Npad, cin_pad, dt, s, bke(dt)));
    }
    nparams += (int64_t)Co * Ci * k * k;
    const std::string bkey = prefix + ".bias";
    return padded_bias(has_bias ? &bkey : nullptr, Co, Npad, &out->bias);
  }
  // Linear layers `wkeys` [Nper][K] each (+ `bkeys`, or none), stacked on N, with the LayerNorm (gamma, beta) in front of them
  // folded in: launch_ln_fold's format.  n_valid: output columns of the launch (half the rows for a GEGLU projection)
  int ln_linear(const float* gamma, const float* beta, const std::vector<std::string>& wkeys, const std::vector<std::string>& bkeys,
                int Nper, int K, int Npad, int n_valid, const std::vector<int>* row_map, float scale, ConvW* out) {
    LnFold f;
    f.parts = (int)wkeys.size(); f.Nper = Nper; f.K = K; f.Npad = Npad;
    f.gamma = gamma; f.beta = beta; f.row_map = row_map; f.scale = scale; f.dtype = dt;
    for (int i = 0; i < f.parts; ++i) {
      TRY(wm->get(wkeys[i], (int64_t)Nper * K, &f.w[i]));
      if (!bkeys.empty()) TRY(wm->get(bkeys[i], Nper, &f.bias[i]));
      nparams += (int64_t)Nper * K + (bkeys.empty() ? 0 : Nper);
    }
    out->N = Npad; out->n_valid = n_valid; out->cin_pad = K; out->taps = 1; out->cout = n_valid;
    TRY(arena->alloc(&out->w, (size_t)Npad * K * esize(dt)));
    weights(out->w, (size_t)Npad * K);
    // one scratch for the folds of a handle, grown when a larger one comes (every use is ordered on the builder's stream)
    if (const size_t need = ln_fold_scratch_bytes(f); need > fold_cap) {
      HIP_TRY(hipMalloc(&fold_scratch, need));
      temps.push_back(fold_scratch);
      fold_cap = need;
    }
    void *pc1, *pc2;
    TRY(arena->alloc(&pc1, (size_t)Npad * sizeof(float)));
    TRY(arena->alloc(&pc2, (size_t)Npad * sizeof(float)));
    out->c1 = (float*)pc1;
    out->bias = (float*)pc2;
    return launch_code(launch_ln_fold(f, fold_scratch, out->w, out->c1, out->bias, s), "launch_ln_fold failed");
  }
  int upload_ints(const std::vector<int>& v, int** dev) {
    void* p;
    HIP_TRY(hipMalloc(&p, v.size() * sizeof(int)));
    temps.push_back(p);
    HIP_TRY(hipMemcpyAsync(p, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice, s));
    *dev = (int*)p;
    return 0;
  }
  int finish(HandleBase& h) {
    // (after every row sum / bias that is computed FROM the packed matrices: the folded-LayerNorm c1 vectors)
    for (const auto& e : x3_w) TRY(launch_split_planes(e.first, e.second, s));
    x3_w.clear();
    HIP_TRY(hipStreamSynchronize(s));
    for (void* p : temps) (void)hipFree(p);
    temps.clear();
    h.nparams = nparams;
    return 0;
  }
};

// ------------------------------------------------------------------ executor helpers
struct Act {
  void* p = nullptr;
  int C = 0, H = 0, W = 0;
};

// what differs between the Linear launches of Exec::linear
struct LinearOpt {
  const float* rowstats = nullptr;   // [M][2] from Exec::rowstats(): the ConvW holds a folded LayerNorm
  const void* resid = nullptr;       // [M][ldo], may be the output itself
  int epi = EPI_STORE;
  int silu = 0;
};

// what differs between the conv launches of Exec::conv
struct ConvOpt {
  const Act* x2 = nullptr;           // channel-concatenated behind x
  int stride = 1;
  int up = 0;                        // nearest x2 in front of the conv
  bool persist = true;               // the output is kept (false: on the scratch stack)
  const float* rowbias = nullptr;    // per-image row added to the bias (time embedding), rb_stride floats apart
  int rb_stride = 0;
  const Act* resid = nullptr;
  int silu = 0;
  int pad = -1;                      // stride 2: -1 = pad 1 both sides, 0 = pad 0 + one zero row/column at the bottom/right
  void* dst = nullptr;               // the output goes there (memory the caller owns, [B, Ho*Wo, n_valid]) instead of into the workspace
};

struct Exec {
  Workspace* ws;
  int dt;
  int B;
  hipStream_t s;
  int attn_fp8_min_tokens = 0;
  void* gn_sync = nullptr;     // the handle's hand-off region of the cooperative GroupNorm (gn_sync_bytes())
  int gn_poll_us = -1;         // >= 0: poll bound of this handle's cooperative norms (backing off, see unet.hip sample_steps)
  int x3 = 0;                  // fp32 handles in LDMSEG_BF16X3 mode: IgemmParams::x3 of every GEMM launch
  void* cf_sync = nullptr;     // the handle's counter region of the in-launch split-K finish (igemm_cf_bytes())
  bool dry() const { return ws->dry; }
  // a request beyond the planned workspace (a plan made under other tuning knobs): fail before anything is launched on it
  int ws_ok() const { return ws->overflow ? fail(LDMSEG_E_OOM, "workspace plan exceeded (stale plan): nothing was launched") : 0; }

  // Every launch of a pass: nothing in a dry pass, no launch on a stale plan, the launcher code fn() returns as the ABI's (launch_code),
  // and while profiling a record of it (family, flops, bytes and the text label() makes, which is built only then).
  template <typename Label, typename Launch>
  int launch(const char* what, int family, double flops, double bytes, Label&& label, Launch&& fn, const char* arg_what = nullptr) {
    if (dry()) return 0;
    TRY(ws_ok());
    if (!g_prof.on) return launch_code(fn(), what, arg_what);
    ProfFamily& f = g_prof.fam[family];
    f.label.push_back(label());
    f.lflops.push_back(flops);
    f.launches++; f.flops += flops; f.bytes += bytes;
    const hipEvent_t a = g_prof.get(), b = g_prof.get();
    (void)hipEventRecord(a, s);
    const int r = fn();
    (void)hipEventRecord(b, s);
    f.ev.emplace_back(a, b);
    return launch_code(r, what, arg_what);
  }

  Act new_act(int C, int H, int W, bool persist) {
    Act a;
    a.C = C; a.H = H; a.W = W;
    const size_t bytes = (size_t)B * H * W * C * esize(dt);
    a.p = persist ? ws->persist(bytes) : ws->scratch(bytes);
    return a;
  }

  int igemm(IgemmParams& p) {
    p.cf_ctr = (unsigned long long*)cf_sync;
    if (p.splits == 1) {
      const int sp = igemm_plan_splits(p, dt);
      if (sp > 1) {
        p.splits = sp;
        p.partial = (float*)ws->scratch((size_t)sp * p.M * p.N * sizeof(float));
      }
    }
    // GEGLU: n_valid counts the OUTPUT channels, the GEMM computes value and gate columns for each
    const double ncols = (p.epi == EPI_GEGLU) ? 2.0 * p.n_valid : (double)p.n_valid;
    const int ktot = p.taps * (p.C0 + p.C1) + p.C2 + p.C3;
    const double flops = 2.0 * p.M * ncols * ktot;
    const double bytes = ((double)p.M * (p.C0 + p.C1 + p.C2 + p.C3) + (double)p.N * ktot + (double)p.M * p.n_valid) * esize(dt);
    auto label = [&] {
      return "M=" + std::to_string(p.M) + " N=" + std::to_string((int)ncols) + " K=" + std::to_string(ktot) + (p.C2 ? "(+1x1 " + std::to_string(p.C2 + p.C3) + ")" : "") +
             " taps=" + std::to_string(p.taps) + " stride=" + std::to_string(p.stride) + " up=" + std::to_string(p.up) +
             " epi=" + std::to_string(p.epi) + " splits=" + std::to_string(p.splits);
    };
    return launch("launch_igemm failed", 0, flops, bytes, label, [&] {
      p.x3 = (dt == DT_F32) ? ((p.w_dynamic && x3) ? 1 : x3) : 0;      // (W = an activation tensor: split in the K loop)
      return launch_igemm(p, dt, s);
    });
  }

  // conv3x3 / 1x1 over NHWC `x`
  int conv(const ConvW& w, const Act& x, Act* out, const ConvOpt& o = {}) {
    const int ctot = x.C + (o.x2 ? o.x2->C : 0);
    if (ctot != w.cin_pad) return fail(LDMSEG_E_SHAPE, "conv: channel mismatch");
    if (o.up && w.w_up4 && w.taps == 9 && o.stride == 1 && !o.x2 && !o.resid && !o.rowbias && !o.silu && o.pad < 0 && !o.dst &&
        igemm_up4_ok(B, x.H, x.W, x.C, w.N, dt)) {
      // conv3x3(nearest_x2(x)) as four 2x2 phase convs on the low-resolution map: 4 B H W virtual rows, K = 4 C
      *out = new_act(w.n_valid, 2 * x.H, 2 * x.W, o.persist);
      IgemmParams p;
      p.src0 = x.p; p.C0 = x.C;
      p.B = B; p.Hi = p.Ho = x.H; p.Wi = p.Wo = x.W;
      p.taps = 4; p.stride = 1; p.up4 = 1;
      p.M = 4 * B * x.H * x.W; p.N = w.N; p.n_valid = w.n_valid;
      p.W = w.w_up4; p.bias = w.bias;
      p.out = out->p; p.ldo = w.n_valid;
      p.epi = EPI_STORE;
      return igemm(p);
    }
    const int Hl = o.up ? 2 * x.H : x.H, Wl = o.up ? 2 * x.W : x.W;
    // stride 2: pad 1 both sides (UNet downsample_padding=1) or pad 0 + one zero row/column at the bottom/right
    const int Ho = (w.taps == 9 && o.stride == 2) ? (o.pad == 0 ? Hl / 2 : (Hl - 1) / 2 + 1) : Hl;
    const int Wo = (w.taps == 9 && o.stride == 2) ? (o.pad == 0 ? Wl / 2 : (Wl - 1) / 2 + 1) : Wl;
    if (o.dst) { out->p = o.dst; out->C = w.n_valid; out->H = Ho; out->W = Wo; }
    else *out = new_act(w.n_valid, Ho, Wo, o.persist);
    IgemmParams p;
    p.src0 = x.p; p.C0 = x.C;
    if (o.x2) { p.src1 = o.x2->p; p.C1 = o.x2->C; }
    p.B = B; p.Hi = x.H; p.Wi = x.W; p.Ho = Ho; p.Wo = Wo;
    p.taps = w.taps; p.stride = o.stride; p.up = o.up; p.pad = o.pad;
    p.M = B * Ho * Wo; p.N = w.N; p.n_valid = w.n_valid;
    p.W = w.w; p.bias = w.bias;
    if (w.w_cm && o.pad < 0 && igemm_conv_cm(x.H * x.W, ctot, w.N, 3, o.stride, o.up, dt)) { p.W = w.w_cm; p.cm = 1; }
    p.rowbias = o.rowbias; p.rb_stride = o.rb_stride;
    if (o.resid) { p.resid = o.resid->p; p.ldr = o.resid->C; }
    p.out = out->p; p.ldo = w.n_valid;
    p.epi = EPI_STORE; p.silu = o.silu;
    return igemm(p);
  }

  // A GEMM over the B x H x W map `src` (C stored channels a pixel) with `w` as packed, into memory the caller names, for the
  // launches Exec::conv does not make: a head conv into caller memory (EPI_NCHW_F32: fp32 NCHW, or EPI_STORE rows of n_valid),
  // the ConvTranspose2d scatter (EPI_CONVT2: rows of w.cout on the 2H x 2W map), a data gradient on its own packing (no bias).
  int gemm(const ConvW& w, const void* src, int C, int H, int W, void* out, int epi) {
    IgemmParams p;
    p.src0 = src; p.C0 = C; p.B = B; p.Hi = p.Ho = H; p.Wi = p.Wo = W;
    p.taps = w.taps; p.M = B * H * W; p.N = w.N; p.n_valid = w.n_valid;
    p.W = w.w; p.bias = w.bias;
    p.out = out; p.epi = epi;
    if (epi == EPI_CONVT2) p.ldo = p.cout = w.cout;
    else if (epi != EPI_NCHW_F32) p.ldo = w.n_valid;
    return igemm(p);
  }

  // Linear over token rows: out[B * Hi * Wi][ldo] = src[.][K] w^T + bias.  (Hi, Wi) is the row geometry of the launch: the map of a
  // UNet level, (tokens, 1) elsewhere.  A folded LayerNorm (o.rowstats) reads its row sums from the ConvW.
  int linear(const ConvW& w, const void* src, int K, int Hi, int Wi, void* out, int ldo, const LinearOpt& o = {}) {
    // (the callers size `out` by ldo, the kernel stores w.n_valid columns)
    if (K != w.cin_pad || w.taps != 1 || ldo != w.n_valid || (o.rowstats && !w.c1)) return fail(LDMSEG_E_SHAPE, "linear: shape mismatch");
    IgemmParams g;
    g.src0 = src; g.C0 = K; g.B = B; g.Hi = g.Ho = Hi; g.Wi = g.Wo = Wi;
    g.M = B * Hi * Wi; g.N = w.N; g.n_valid = w.n_valid; g.W = w.w; g.bias = w.bias;
    if (o.rowstats) { g.rowstats = o.rowstats; g.c1 = w.c1; }
    if (o.resid) { g.resid = o.resid; g.ldr = ldo; }
    g.out = out; g.ldo = ldo; g.epi = o.epi; g.silu = o.silu;
    return igemm(g);
  }

  // resnet tail: out = conv2(h) + conv_shortcut(cat([x, x2])) as one launch (ResnetW::conv2x); false = the launch has no
  // extra-tap form here (fp32, debug key 19 off, a forced tile policy ...): the caller runs the two convs
  bool conv_xt_ok(const ConvW& w, const Act& h, const Act& x, const Act* x2) const {
    if (!w.w || x.C + (x2 ? x2->C : 0) != w.xt_cin) return false;      // (a mismatch takes the two-conv path, which reports it)
    IgemmParams p;
    p.C0 = h.C; p.taps = 9; p.N = w.N; p.src2 = x.p ? x.p : (const void*)1; p.C2 = x.C;
    if (x2) { p.src3 = x2->p ? x2->p : (const void*)1; p.C3 = x2->C; }
    return igemm_xt_ok(p, dt);
  }
  int conv_xt(const ConvW& w, const Act& h, const Act& x, const Act* x2, Act* out) {
    if (h.C != w.cin_pad) return fail(LDMSEG_E_SHAPE, "conv_xt: channel mismatch");
    // the weight rows are [9 cout | xt_cin] long: a shortcut input of another width would walk off them
    if (x.C + (x2 ? x2->C : 0) != w.xt_cin) return fail(LDMSEG_E_SHAPE, "conv_xt: shortcut channel mismatch");
    *out = new_act(w.n_valid, h.H, h.W, true);
    IgemmParams p;
    p.src0 = h.p; p.C0 = h.C;
    p.src2 = x.p; p.C2 = x.C;
    if (x2) { p.src3 = x2->p; p.C3 = x2->C; }
    p.B = B; p.Hi = p.Ho = h.H; p.Wi = p.Wo = h.W;
    p.taps = 9; p.stride = 1; p.up = 0; p.pad = -1;
    p.M = B * h.H * h.W; p.N = w.N; p.n_valid = w.n_valid;
    p.W = w.w; p.bias = w.bias;
    p.out = out->p; p.ldo = w.n_valid;
    p.epi = EPI_STORE;
    return igemm(p);
  }

  // 3x3 conv (stride 1, time-embedding row) whose only consumer is a GroupNorm (resnet conv1 -> norm2): where the conv runs
  // as K slices and the map is small, the slices' finish and the norm are one launch and the conv's own output is never
  // stored (launch_finish_groupnorm); otherwise conv and norm as usual.
  int conv_groupnorm(const ConvW& w, const Act& x, const float* rowbias, int rb_stride, const NormW& n, float eps, int silu,
                           Act* out) {
    if (x.C != w.cin_pad || n.C != w.n_valid) return fail(LDMSEG_E_SHAPE, "conv_groupnorm: channel mismatch");
    IgemmParams p;
    p.src0 = x.p; p.C0 = x.C;
    p.B = B; p.Hi = x.H; p.Wi = x.W; p.Ho = x.H; p.Wo = x.W;
    p.taps = w.taps; p.stride = 1; p.up = 0; p.pad = -1;
    p.M = B * x.H * x.W; p.N = w.N; p.n_valid = w.n_valid;
    p.W = w.w; p.bias = w.bias;
    p.rowbias = rowbias; p.rb_stride = rb_stride;
    p.epi = EPI_STORE;
    const int sp = igemm_plan_splits(p, dt);
    // round 6 (debug key 23 bit 2, default on): where the conv finishes its K slices inside the launch - bf16, 256-row tiles, i.e. the
    // 16x16 maps at B = 8 - run conv + GroupNorm (gn_group_kernel: 5 us) instead of slabs + the fused finish-GroupNorm launch (16 us):
    // measured -12 us per forward in one process (7.963 -> 7.951 ms); on the 128-row tiles of the 8x8 maps the fused launch stays
    const bool conv_then_gn = sp >= 2 && dt == DT_BF16 && (igemm_get_cf_mode() & 5) == 5 && p.M >= 2048 && p.M % 256 == 0;
    if (sp < 2 || conv_then_gn || !finish_groupnorm_ok(B, x.H * x.W, w.n_valid, dt)) {
      Act h;
      ConvOpt o;
      o.persist = false; o.rowbias = rowbias; o.rb_stride = rb_stride;
      TRY(conv(w, x, &h, o));
      return groupnorm(n, h, nullptr, eps, silu, out);
    }
    *out = new_act(w.n_valid, x.H, x.W, false);
    if (w.w_cm && igemm_conv_cm(x.H * x.W, x.C, w.N, 3, 1, 0, dt)) { p.W = w.w_cm; p.cm = 1; }
    p.splits = sp;
    p.partial = (float*)ws->scratch((size_t)sp * p.M * p.N * sizeof(float));
    p.no_finish = 1;
    TRY(igemm(p));
    GNParams g;
    g.src0 = nullptr; g.C0 = w.n_valid; g.B = B; g.HW = x.H * x.W; g.groups = 32;
    g.gamma = n.g; g.beta = n.b; g.eps = eps; g.silu = silu;
    g.out = out->p;
    const double bytes = ((double)sp * p.M * p.N * sizeof(float)) + (double)p.M * w.n_valid * esize(dt);
    return launch("launch_finish_groupnorm failed", 2, 0, bytes, [&] { return "finish+GN HW=" + std::to_string(g.HW) + " C=" + std::to_string(g.C0); },
                  [&] { return launch_finish_groupnorm(p, g, dt, s); });
  }

  int groupnorm(const NormW& n, const Act& x, const Act* x2, float eps, int silu, Act* out) {
    const int ctot = x.C + (x2 ? x2->C : 0);
    if (ctot != n.C) return fail(LDMSEG_E_SHAPE, "groupnorm: channel mismatch");
    *out = new_act(ctot, x.H, x.W, false);
    GNParams g;
    g.src0 = x.p; g.C0 = x.C;
    if (x2) { g.src1 = x2->p; g.C1 = x2->C; }
    g.B = B; g.HW = x.H * x.W; g.groups = 32;
    g.gamma = n.g; g.beta = n.b; g.eps = eps; g.silu = silu;
    g.out = out->p;
    g.nchunk = gn_nchunk(B, g.HW);
    g.sync_region = gn_sync;
    g.poll_us = gn_poll_us;
    g.partial = (float*)ws->scratch((size_t)B * g.nchunk * 32 * 2 * sizeof(float));
    return launch("launch_groupnorm failed", 2, 0, 3.0 * B * g.HW * ctot * esize(dt), [&] { return "HW=" + std::to_string(g.HW) + " C=" + std::to_string(ctot); },
                  [&] { return launch_groupnorm(g, dt, s); });
  }

  // GroupNorm statistics only ({mean, M2} per image, pixel chunk and group): the consumer (tproj.hip) combines and applies them
  int groupnorm_stats(const NormW& n, const Act& x, float eps, GnFold* gf) {
    if (x.C != n.C) return fail(LDMSEG_E_SHAPE, "groupnorm: channel mismatch");
    GNParams g;
    g.src0 = x.p; g.C0 = x.C;
    g.B = B; g.HW = x.H * x.W; g.groups = 32;
    g.nchunk = g_gnfold_mode > 1 ? (g_gnfold_mode > 64 ? 64 : g_gnfold_mode) : proj_qkv_gn_chunks(B, g.HW);
    g.partial = (float*)ws->scratch((size_t)B * g.nchunk * 32 * 2 * sizeof(float));
    gf->partial = g.partial; gf->gamma = n.g; gf->beta = n.b; gf->nchunk = g.nchunk; gf->HW = g.HW; gf->eps = eps;
    return launch("launch_groupnorm_stats failed", 2, 0, 1.0 * B * g.HW * x.C * esize(dt), [&] { return "stats HW=" + std::to_string(g.HW) + " C=" + std::to_string(x.C); },
                  [&] { return launch_groupnorm_stats(g, dt, s); });
  }

  // LayerNorm statistics only (the normalisation itself is folded into the consuming GEMM)
  int rowstats(const Act& x, float eps, float* stats) {
    const int M = B * x.H * x.W;
    return launch("launch_rowstats failed", 3, 0, 1.0 * M * x.C * esize(dt), no_label, [&] { return launch_rowstats(x.p, stats, M, x.C, eps, dt, s); });
  }

  int layernorm(const NormW& n, const Act& x, float eps, int silu, Act* out, bool inplace = false) {
    *out = inplace ? x : new_act(x.C, x.H, x.W, false);
    const int M = B * x.H * x.W;
    return launch("launch_layernorm failed", 3, 0, 2.0 * M * x.C * esize(dt), no_label,
                  [&] { return launch_layernorm(x.p, out->p, n.g, n.b, M, x.C, eps, silu, dt, s); });
  }
};

// the executor of one (dry or real) pass over a handle's workspace
Exec make_exec(HandleBase& h, int B, hipStream_t s, bool dry, size_t scratch_base);

// ------------------------------------------------------------------ the resnet block the UNet and the image VAE share
struct ResnetW {
  NormW norm1, norm2;
  ConvW conv1, conv2, shortcut;
  ConvW conv2x;           // bf16, has_shortcut: conv2 and conv_shortcut as ONE matrix [N][9 cout | cin], bias = b2 + bs (IgemmParams::src2)
  bool has_shortcut = false;
  int cin = 0, cout = 0, temb_off = 0;
};
int build_resnet(Builder& b, const std::string& p, int cin, int cout, int* temb_off, ResnetW* r);

// ------------------------------------------------------------------ workspace planning
int ensure_ws(HandleBase& h, size_t need);

// Measure a pass (impl(dry = true, 0)) and make the workspace large enough for it.  key: the shape numbers the dry run depends on
// besides the handle itself - the plan is then kept until they or g_plan_epoch change; null = measure on every call.
template <typename Impl>
int plan_workspace(HandleBase& h, const PlanKey* key, Impl&& impl) {
  int k[5] = {0, 0, 0, 0, g_plan_epoch};
  if (key) std::copy(key->begin(), key->end(), k);
  if (!key || !h.plan_valid || !std::equal(k, k + 5, h.plan_key)) {
    h.plan_valid = false;
    TRY(impl(true, (size_t)0));
    h.plan_persist = rup(h.ws.persist_peak, 4096);
    h.plan_scratch = rup(h.ws.scratch_peak, 4096);
    std::copy(k, k + 5, h.plan_key);
    h.plan_valid = key != nullptr;
  }
  return ensure_ws(h, h.plan_persist + h.plan_scratch);
}
// ... and run it.  A host allocation failure inside a pass (labels, the skip stack) ends here, not in the caller's C frame.
template <typename Impl>
int plan_and_run(HandleBase& h, const PlanKey* key, Impl&& impl) {
  try {
    TRY(plan_workspace(h, key, impl));
    return impl(false, h.plan_persist);
  } catch (...) {
    return fail(LDMSEG_E_OOM, "host allocation failed");
  }
}

// ------------------------------------------------------------------ handles
int check_arch(int device);
int make_weight_map(int n, const char* const* names, const void* const* ptrs, const int64_t* numels, WeightMap* wm);

// *_create of every handle type: the argument checks all share, `check(cfg)` for the type's own, then the handle on cfg->device:
// parameters (build), the GEMM launcher's per-device state and the hand-off regions.  Nothing is left behind on an error.
template <typename H, typename Cfg, typename Check>
int create_handle(const Cfg* cfg, int n_weights, const char* const* names, const void* const* dev_ptrs, const int64_t* numels,
                  Check&& check, int (*build)(H*, const WeightMap&), bool needs_gn_sync, H** out) {
  g_err.clear();
  if (!cfg || !out) return fail(LDMSEG_E_ARG, "null argument");
  if (cfg->compute_dtype != LDMSEG_F32 && cfg->compute_dtype != LDMSEG_BF16 && cfg->compute_dtype != LDMSEG_BF16X3) return fail(LDMSEG_E_ARG, "bad compute_dtype");
  TRY(check(*cfg));
  DeviceGuard dg(cfg->device);
  TRY(check_arch(cfg->device));
  H* h = nullptr;
  int r = 0;
  try {
    WeightMap wm;
    TRY(make_weight_map(n_weights, names, dev_ptrs, numels, &wm));
    h = new H();
    h->cfg = *cfg;
    h->device = cfg->device;
    h->dt = cfg->compute_dtype == LDMSEG_BF16 ? DT_BF16 : DT_F32;
    h->x3 = cfg->compute_dtype == LDMSEG_BF16X3;
    r = build(h, wm);
  } catch (...) {
    r = fail(LDMSEG_E_OOM, "host allocation failed while building the handle");
  }
  if (r == 0) r = igemm_warm();
  if (r == 0 && needs_gn_sync) r = alloc_gn_sync(&h->gn_sync);
  if (r == 0) r = alloc_cf_sync(&h->cf_sync);
  if (r != 0) { delete h; return r; }
  *out = h;
  return 0;
}

// the two ABI entries every handle type has besides its *_create
#define LDMSEG_HANDLE_ABI(T)                        \
  void T##_destroy(T* h) { delete h; } \
  int64_t T##_num_params(const T* h) { return h ? h->nparams : 0; }

}  // namespace ldmseg::rt
