// Host-side launch API of the gfx950 kernels (internal; the public boundary is
// include/ldmseg_hip.h).  All tensors are NHWC ("[B, H*W, C]") in the compute
// dtype (bf16 or f32) unless a name says otherwise.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "igemm_types.h"   // DType, Epilogue, IgemmDispatch, IgemmLaunchDesc

namespace ldmseg {

// Exact n / d for 0 <= n < 2^31 by one v_mul_hi_u32 and a shift (Granlund-Montgomery: s = ceil(log2 d),
// M = ceil(2^(31+s) / d) < 2^32, q = (n * M) >> (31 + s)).  A runtime integer division is a ~40-instruction VALU sequence
// on this part; kernels whose first useful instruction sits behind several of them (row -> (image, y, x) of every gathered
// row, item -> tile) pay microseconds per launch for it.  Divisors come from the host, made by fastdiv_make().
struct FastDiv {
  unsigned mul = 0;     // 0: divisor is 1
  int shift = 0;        // applied to the high word
  int d = 1;
};
inline FastDiv fastdiv_make(int d) {
  FastDiv f;
  f.d = d < 1 ? 1 : d;
  if (f.d == 1) return f;
  int s = 0;
  while ((1ll << s) < f.d) ++s;
  const unsigned long long num = 1ull << (31 + s);
  f.mul = (unsigned)((num + (unsigned long long)f.d - 1) / (unsigned long long)f.d);
  f.shift = s - 1;
  return f;
}

struct IgemmParams {
  const void* src0 = nullptr;  // [B, Hi*Wi, C0]
  const void* src1 = nullptr;  // [B, Hi*Wi, C1]  channel-concat partner (torch.cat([h, skip],1))
  int C0 = 0, C1 = 0;
  // Extra centre tap (round 5): K continues past the 3x3 taps with C2 (+ C3) channels of a THIRD (and fourth) tensor read at the
  // output pixel itself - a 1x1 conv over torch.cat([src2, src3], 1) accumulated into the same tile.  The resnet's
  // conv_shortcut(x) + conv2(h) of diffusers' ResnetBlock2D as ONE launch: W rows are [9 * (C0 + C1) | C2 + C3], bias = b2 + bs.
  // 3x3, stride 1, no upsample, tap-major K, bf16 only (launch_igemm checks).
  const void* src2 = nullptr;
  const void* src3 = nullptr;
  int C2 = 0, C3 = 0;
  int B = 0, Hi = 0, Wi = 0, Ho = 0, Wo = 0;
  int taps = 1;     // 1 (1x1 conv / Linear) or 9 (3x3, pad 1)
  int pad = -1;     // top/left zero padding of a 3x3 conv; -1 = 1.  0 with stride 2 = F.pad(x,(0,1,0,1)) + conv(pad 0)
                    // (diffusers Downsample2D(padding=0) of the AutoencoderKL encoder); the bottom/right edge is bounds-checked
  int stride = 1;   // 1 | 2
  int up = 0;       // nearest x2 upsample folded into the gather (Upsample2D)
  // up4 (round 5): conv3x3(nearest_x2(x)) as four 2x2-tap phase convs on the LOW-resolution map.  An output pixel (2i + py, 2j + px)
  // of the upsampled map only ever sees 2 x 2 distinct source pixels - rows {i-1, i} (py = 0) or {i, i+1} (py = 1), columns
  // likewise - so the nine taps collapse into four with pre-summed weights: K = 4 C instead of 9 C, 2.25 x fewer MACs, same
  // result up to the rounding of the summed weights.  The launch walks 4 * B * Hi * Wi virtual rows ordered (phase, image, i, j);
  // taps = 4, Hi = Ho, Wi = Wo = the low-resolution map, W = [4 phases][N][4 taps][C], out = [B, 2Hi * 2Wi, ldo].
  int up4 = 0;
  int cm = 0;       // 3x3 only: W is packed in channel-major K order, k = (channel tile, tap, channel in tile), instead of
                    // (tap, channel); needs stride 1, pad 1, no upsample (launch_igemm checks)
  int M = 0;        // B*Ho*Wo
  int N = 0;        // packed rows of W (multiple of the N tile)
  int n_valid = 0;  // real output channels (store mask)
  const void* W = nullptr;       // [N][taps*(C0+C1)] compute dtype, K = (tap, channel)
  const float* bias = nullptr;   // [N] (packed order) or null
  const float* rowbias = nullptr;  // [B][rb_stride] per-image bias (time embedding) or null
  int rb_stride = 0;
  // LayerNorm folded into the GEMM (transformer norm1 -> q|k|v, norm3 -> GEGLU): X is the un-normalised tensor, W holds
  // gamma_k * W[n][k], c1[n] = sum_k W[n][k] of that packed matrix, bias[n] = sum_k beta_k W0[n][k] + b[n], and
  // out = rstd_m * (acc - mean_m * c1[n]) + bias[n] with (mean_m, rstd_m) = rowstats[m] from launch_rowstats.
  const float* rowstats = nullptr;   // [M][2] or null
  const float* c1 = nullptr;         // [N]
  const void* resid = nullptr;   // [M][ldr] residual, compute dtype, may alias out
  int ldr = 0;
  void* out = nullptr;
  int ldo = 0;
  int epi = EPI_STORE;
  int silu = 0;
  int cout = 0;     // EPI_CONVT2: real Cout per tap
  // split-K: when splits>1 partial sums go to `partial` [splits][M][N] f32 and
  // igemm_splitk_finish applies the epilogue.
  int splits = 1;
  float* partial = nullptr;
  int no_finish = 0;             // splits > 1: leave the slabs as they are, the caller runs its own finish (launch_finish_groupnorm)
  // In-launch cooperative finish (round 6): cf_ctr = the caller's counter region (igemm_cf_bytes() bytes, zeroed once; a handle
  // owns one; launches that share a region must be ordered on one stream) or null = two launches as before.  The launcher decides
  // per launch (every K slice of every tile must have its own co-resident workgroup) and sets cf / cf_bytes / cf_poll_ticks.
  unsigned long long* cf_ctr = nullptr;
  int cf = 0;
  unsigned cf_bytes = 0;         // bytes of the slab set (buffer range of the write-through stores / loads)
  int cf_poll_ticks = 20000;     // bound of the partner poll in 100 MHz ticks
  int cf_diag = 0;               // index of the region's diagnostics word (workgroups that gave up waiting)
  const void* zeros = nullptr;   // >= 16 B of zeros (set by the launcher)
  // set by the launcher: divisions the kernels need (by Ho*Wo, Wo, the number of n tiles / tiles / K slices, K tiles per tap)
  FastDiv fd_hwo, fd_wo, fd_nt, fd_ntiles, fd_nsplit, fd_tpt, fd_mphase;
  int x3 = 0;                    // fp32 launches only: split-bf16 arithmetic (hi + lo, three bf16 MFMAs per product block) instead of
                                 // the exact fp32 MFMA - compute_dtype "bf16x3" of the handles.  2 (round 6): W already holds the
                                 // hi | lo planes (launch_split_planes at create time): no weight split in the K loop
  int w_dynamic = 0;             // host-side: W is an activation tensor of this call (image-VAE attention), never pre-split
  int dbg = 0;                   // ablation flags for profiling experiments (results are wrong when != 0)
  unsigned long long* ts = nullptr;   // LDMSEG_IGEMM_ABLATE builds: per-workgroup s_memtime stamps (wave 0)
};

// returns 0 or a negative error (bad shape)
int launch_igemm(const IgemmParams& p, int dtype, hipStream_t s);
size_t igemm_partial_bytes(const IgemmParams& p);
int igemm_warm();   // per-device lazy state (zero page) created now instead of inside the first launch
int num_cus();      // compute units of the current device
int igemm_plan_splits(const IgemmParams& p, int dtype);
// cooperative split-K finish inside the igemm launch (IgemmParams::cf_ctr).  Region size; debug key 23: bit 0 = on for the 256-row
// tile forms (default, with bit 2: engine.hip conv_groupnorm), bit 3 = on for every tile form with the instantiation, bit 1 = zero-length poll (every workgroup that is not
// the last arriver gives up: the last arriver reduces the whole tile), bits 8.. = poll bound in microseconds (0 = default 200);
// fallbacks are counted in the region's last word.
size_t igemm_cf_bytes();
void igemm_set_cf_mode(int mode);
int igemm_get_cf_mode();
// tuning (debug key 24): >= 0 = every plain-store launch runs entry (v & 0xff) of the instantiation list with (v >> 8) K slices, as
// if the launch table held that entry for its shape (unlike key 5 this keeps the extra-tap / launch-table routes); -1 = off
void igemm_set_table_override(int v);
void attention_set_qf1(int v);    // tuning knob: force 16 query rows per wave
void igemm_set_tsbuf(void* dev_buf);   // LDMSEG_IGEMM_ABLATE builds only
void igemm_set_dbg(int flags);
void ops_bench_knob(int key, int value);   // ldmseg_bench_igemm (ops_api.hip): 6 = number of weight copies rotated, 7 = folded-LN launch
// K order a 3x3 conv launch uses: -1 = the shipped rule (channel-major for stride-1 convs without upsample on maps of
// >= 4096 pixels with >= 640 input channels: there one tap sweep over the X operand no longer fits an XCD's L2 and the
// channel-major order measured -6 %; smaller launches measured +2..8 % and keep the tap-major order), 0 = tap-major
// everywhere, 1 = channel-major wherever the kernel supports it.  Layers that can meet the rule hold both packings.
void igemm_set_cm_mode(int mode);
int igemm_get_cm_mode();
bool igemm_conv_cm(int hw, int ctot, int n, int k, int stride, int up, int dtype);
// conv3x3 on a nearest-x2 upsampled map as four 2x2 phase convs (IgemmParams::up4): whether the layer shape / map size has the
// launch and debug key 21 allows it, and the weight packing it reads ([4][Npad][4][Cipad] from OIHW fp32)
bool igemm_up4_ok(int B, int H, int W, int C, int N, int dtype);
void igemm_set_up4_mode(int on);
int igemm_get_up4_mode();
int launch_pack_up4(const float* w, void* out, int Co, int Ci, int Npad, int Cipad, int dtype, hipStream_t s);
bool igemm_xt_ok(const IgemmParams& p, int dtype);   // the launch (with src2 / C2 set) has an extra-tap instantiation and key 19 allows it
void igemm_set_xt_mode(int on);
int igemm_get_xt_mode();
// out[n][0:K1] = a[n][:], out[n][K1:K1+K2] = b[n][:]  (rows of two packed weight matrices side by side), compute dtype
// Weights of two chained Linear layers with nothing in between, y = Wp (W2 g + b2 + h) + bp = [Wp W2 | Wp] [g | h] + (bp + Wp b2):
// wcat [C][5C] fp32 = [Wp W2 | Wp], bcat [C] = bp + Wp b2 (wp [C][C], w2 [C][4C]; fp32 products, create time only)
int launch_chain_weights(const float* wp, const float* w2, const float* b2, const float* bp, float* wcat, float* bcat, int C, hipStream_t s);
int launch_vec_add(const float* a, const float* b, float* out, int n, hipStream_t s);
// packed fp32 weights [rows][K] -> split-bf16 planes in place (IgemmParams::x3 == 2); nfloats a multiple of 32
int launch_split_planes(void* w, size_t nfloats, hipStream_t s);
int launch_concat_rows(const void* a, int K1, const void* b, int K2, void* out, int N, int dtype, hipStream_t s);
void igemm_force_cfg(int cfg);   // tuning tool: >= 0 runs every launch with that entry of the instantiation list, -1 = off
int igemm_get_dbg();       // current (policy << 8) | ablation flags
int igemm_default_dbg();   // the shipped value
// template instantiation + plan of the most recent launch_igemm (test introspection), and of a launch that is only described
IgemmDispatch igemm_last_dispatch();
int igemm_plan(const IgemmLaunchDesc& desc, int dtype, int cus, IgemmDispatch* d);
std::string igemm_dispatch_name(const IgemmDispatch& d);
std::string igemm_dispatch_line(const IgemmDispatch& d);   // name + " splits=S grid=G"
// the dispatch log: level 0 = off; 1 = the GEMM family (igemm instantiations, the fused GEMM kernels of tfuse / tproj / tail);
// 2 = every kernel of the forward path (+ split-K finish, GroupNorm, LayerNorm statistics, attention).  Enabling clears it.
void igemm_log_enable(int level);
int igemm_log_level();
void igemm_log_note(const char* name);   // recorded while logging is on
std::string igemm_log_read();       // newline-separated
std::string launch_name(const char* fmt, ...);          // printf into a std::string (the names below)
template <typename T>
constexpr const char* dtype_tag() { return sizeof(T) == 2 ? "bf16" : "f32"; }
// Every kernel launch of the forward path goes through one of these: NAME - the kernel with every template argument and the
// run-time form that changes the code it runs, so that two launches executing different code never share a name - is recorded
// in the dispatch log (evaluated only while the log is at LEVEL or above), then the kernel is launched.  LDMSEG_LAUNCH_GEMM: the
// GEMM family (log level 1); LDMSEG_LAUNCH: every other kernel (level 2).  tests/test_launch_sites_cpu.py rejects bare
// hipLaunchKernelGGL calls in those sources outside its allow-list.
#define LDMSEG_LAUNCH_AT(LEVEL, NAME, ...)                                                                  \
  do {                                                                                                      \
    if (::ldmseg::igemm_log_level() >= (LEVEL)) ::ldmseg::igemm_log_note(std::string(NAME).c_str());        \
    hipLaunchKernelGGL(__VA_ARGS__);                                                                        \
  } while (0)
#define LDMSEG_LAUNCH_GEMM(NAME, ...) LDMSEG_LAUNCH_AT(1, NAME, __VA_ARGS__)
#define LDMSEG_LAUNCH(NAME, ...) LDMSEG_LAUNCH_AT(2, NAME, __VA_ARGS__)
// what every launcher returns after its launches: 0, or -3 when HIP refused one
inline int launch_status() { return hipGetLastError() == hipSuccess ? 0 : -3; }
// tile the launcher would pick (for weight padding): N tile size for a given N.
int igemm_pick_bn(int n_real, int epi);

struct GNParams {
  const void* src0 = nullptr; const void* src1 = nullptr;
  int C0 = 0, C1 = 0, B = 0, HW = 0, groups = 32;
  const float* gamma = nullptr; const float* beta = nullptr;
  float eps = 1e-5f; int silu = 0;
  void* out = nullptr;         // [B, HW, C0+C1]
  float* partial = nullptr;    // workspace [B][nchunk][groups][2]
  int nchunk = 0;
  // filled by launch_groupnorm (host): quantities the kernels would otherwise divide for before their first load
  int cpg = 0, vx = 0, ty = 0, per = 0;                 // channels per group, threads per pixel row, pixel rows per trip, pixels per chunk
  FastDiv fd_cpg, fd_vx, fd_aux;                        // aux: units / vectors per pixel of the small / fused kernels
  double inv_n = 0.0;                                   // 1 / (HW * cpg)
  // cooperative one-pass kernel (gn_coop_kernel).  sync_region: the caller's hand-off region (gn_sync_bytes() bytes, zeroed
  // once by gn_sync_init; a handle owns one) or null = a region of the per-device ring.  The launcher derives the rest.
  void* sync_region = nullptr;
  unsigned long long* sync = nullptr;                   // record granules [slab][8 splits][8 entries]
  unsigned long long* sync_ctr = nullptr;               // per-slab ticket counters (the generation tag is drawn on the device)
  unsigned long long* sync_diag = nullptr;              // workgroups that computed a missing partner's record themselves
  int splits = 1;                                       // workgroups that share one (image, group block)
  int coop_mode = 0;                                    // 1: never poll, always take the self-computing path (tests)
  int poll_ticks = 10000;                               // bound of the partner poll in 100 MHz wall-clock ticks
  int poll_us = -1;                                     // >= 0: this launch's poll bound instead of the process-wide one (a handle backing off)
};
size_t gn_sync_bytes();
int gn_sync_init(void* region, hipStream_t s);
int gn_warm();                                          // per-device ring allocated now instead of inside the first launch
// test / diagnostic knobs of the cooperative kernel: mode 1 = always self-compute, poll_us = bound of the poll (default 100)
void groupnorm_set_coop(int mode, int poll_us);
// workgroups that took the self-computing path since the region was initialised (region null: sum over the ring of the current device)
long long gn_coop_fallbacks(const void* region);
const void* gn_sync_diag_ptr(const void* region);      // device address of a region's 8-byte fallback counter
int gn_nchunk(int B, int HW);
int launch_groupnorm(const GNParams& p, int dtype, hipStream_t s);
// statistics only: p.partial[b][chunk][group] = {mean, M2} of p.nchunk pixel chunks of ceil(HW / nchunk) pixels (gn_partial_kernel);
// out / gamma / beta / silu are not used.  Consumer: launch_proj_qkv_fused with a GnFold (tproj.hip)
int launch_groupnorm_stats(const GNParams& p, int dtype, hipStream_t s);
// Split-K finish of a conv fused with the GroupNorm (+SiLU) that consumes it (resnet conv1 -> norm2 on the 8x8 / 16x16
// maps): out = GN(sum_z partial[z] + bias + rowbias[image]) in ONE launch; the conv's own output is never stored.
// ip: the igemm launch (partial, splits, M, N, n_valid, bias, rowbias, rb_stride); g: B, HW, C0 = channels, gamma, beta,
// eps, silu, out.  finish_groupnorm_ok: whether the shape has an instantiation (otherwise: igemm's finish + launch_groupnorm).
bool finish_groupnorm_ok(int B, int HW, int C, int dtype);
int launch_finish_groupnorm(const IgemmParams& ip, const GNParams& g, int dtype, hipStream_t s);
void groupnorm_set_variant(int v);   // tuning knob (debug key 8): the kGn* bits of gn_plan.h
int groupnorm_knob(int key);         // current value of debug key 8 (variant), 10 (mode) or 11 (poll bound in us)
// what launch_groupnorm / launch_finish_groupnorm would run under the current knobs (gn_plan.h; no device): 0 and *pl, -2, -4
struct GnDesc;
struct GnPlan;
int groupnorm_plan(const GnDesc& q, int cus, bool region_ok, GnPlan* pl);
int finish_groupnorm_plan(int B, int HW, int C, int dtype, GnPlan* pl);

// LayerNorm over the last dim of [M][C] (+ optional SiLU) - also LayerNorm2d in NHWC
int launch_layernorm(const void* x, void* y, const float* gamma, const float* beta, int M, int C,
                     float eps, int silu, int dtype, hipStream_t s);
// what launch_layernorm (q.stats = 0) / launch_rowstats (1) would run under the current knobs (ln_plan.h; no device): 0 and *pl, or -2
struct LnDesc;
struct LnPlan;
int layernorm_plan(const LnDesc& q, LnPlan* pl);

// self-attention on fused qkv [B, N, 3C] (q | k | v, channel = head*d + i) -> out [B, N, C]
// dtype 2 = fp32 tensors with the products as three bf16 MFMAs on hi/lo splits (compute_dtype "bf16x3")
int launch_attention(const void* qkv, void* out, int B, int N, int C, int heads, int dtype, hipStream_t s);
// the same with a causal mask built in the kernel (key j contributes to query i iff j <= i; key tiles above a query block's diagonal
// are skipped): head dim 64 only (C == 64 * heads), any N >= 1 - the CLIP text encoder
int launch_attention_causal(const void* qkv, void* out, int B, int N, int C, int heads, int dtype, hipStream_t s);
// Every attention launcher describes its launch, asks attn_choose (attn_plan.h: the rule, no device) once under attention_knobs()
// - debug keys 2 and 15 - and hands the plan to the file that owns the chosen form; launch_attn_*_plan expand the plan's template
// arguments (-2: no such instantiation).  kv8: scratch of plan.scratch_bytes bytes.
struct AttnKnobs;
struct AttnPlan;
AttnKnobs attention_knobs();
int launch_attn_v1_plan(const AttnPlan& p, const void* qkv, void* out, hipStream_t s);       // attention.hip
int launch_attn3_plan(const AttnPlan& p, const void* qkv, void* out, hipStream_t s);         // attention3.hip
int launch_attn4_plan(const AttnPlan& p, const void* qkv, void* out, hipStream_t s);         // attention4.hip
int launch_attn_fp8_plan(const AttnPlan& p, const void* qkv, void* kv8, void* out, hipStream_t s);      // attention_fp8.hip
int launch_attn_mx_plan(const AttnPlan& p, const void* qkv, void* kv8, void* out, hipStream_t s);       // attention_mx.hip
int launch_attn_cross_plan(const AttnPlan& p, const void* q, const void* kv, void* out, hipStream_t s); // attention_cross.hip

// cross-attention (attention_cross.hip): q [B*N, C], kv = to_k | to_v of the context [B*S, 2C] -> out [B*N, C]; any S >= 1 (keys
// past S masked), head dims 40 / 80 / 160; dtype 0 / 1 / 2 as launch_attention (every product in fp32 on the VALU)
int launch_attention_cross(const void* q, const void* kv, void* out, int B, int N, int S, int C, int heads, int dtype, hipStream_t s);
// fp32 [n] -> compute dtype [n] (the conditioning context at the API boundary)
int launch_rows_to_dtype(const float* x, void* y, size_t n, int dtype, hipStream_t s);

// Row-local fusion of the transformer feed-forward at the 320-channel level (tfuse.hip): LayerNorm_3 -> GEGLU -> ff.net.2 (+h)
// [-> proj_out (+x)] in one launch.  mlp_fused_ok: the shape / dtype has the kernel and the mode (debug key 12) allows it.
bool mlp_fused_ok(int C, int dtype);
bool mlp_fused_proj();                      // mode bit 1: proj_out rides along
void mlp_fused_set_mode(int m);             // bit 0: fuse norm3 -> GEGLU -> ff.net.2; bit 1: + proj_out  (default 3)
int mlp_fused_get_mode();
size_t mlp_fused_stream_bytes(int C);
// w1: packed GEGLU weights [8C][C] (16-row value | gate interleave, gamma folded in), w2: [C][4C], wp: proj_out [C][C]; bf16
int launch_pack_mlp_stream(const void* w1, const void* w2, const void* wp, void* out, int C, hipStream_t s);
// tproj.hip (bf16, C = 320): proj_in -> LayerNorm_1 -> q|k|v of a transformer in one row-local launch (writes h and q|k|v).
// proj_qkv_fused_ok: the shape / dtype has the kernel and the mode (debug key 16) allows it.
bool proj_qkv_fused_ok(int C, int M, int dtype);
void proj_qkv_set_mode(int m);
int proj_qkv_get_mode();
size_t proj_qkv_stream_bytes(int C);
int launch_pack_proj_qkv_stream(const void* wp, const void* wqkv, void* out, int C, hipStream_t s);
// gn != null: x is the transformer's RAW input and its GroupNorm (32 groups, no SiLU) runs inside the kernel from the statistics of
// launch_groupnorm_stats (partial [B][nchunk][32][2]); M % HW == 0, HW % 128 == 0 (proj_qkv_gn_fold_ok)
struct GnFold {
  const float* partial = nullptr;
  const float* gamma = nullptr;
  const float* beta = nullptr;
  int nchunk = 0, HW = 0;
  float eps = 1e-6f;
};
bool proj_qkv_gn_fold_ok(int HW);
int proj_qkv_gn_chunks(int B, int HW);    // nchunk for launch_groupnorm_stats (<= 64: the kernel keeps a lane's records in registers)
int launch_proj_qkv_fused(const void* x, void* h, void* qkv, const void* stream, const float* bias4, const void* zeros, int M, int C, float eps,
                          const GnFold* gn, hipStream_t s);
int launch_mlp_fused(const void* h, void* out, const void* x2, const void* stream, const float* bias1, const float* bias2,
                     const float* bias3, const void* zeros, int M, int C, float eps, int proj, int rows_per_image, hipStream_t s);
void mlp_fused_set_dbg(int flags);          // bit 8: no start-chunk rotation; bits 0-7: phase ablation (LDMSEG_TFUSE_ABLATE builds only)
const void* igemm_zero_page();              // >= 64 KB of zeros on the current device (igemm's padding page)

// per-row (mean, rstd) of [M][C] (LayerNorm statistics, two-pass centred variance) -> stats [M][2] f32
int launch_rowstats(const void* x, float* stats, int M, int C, float eps, int dtype, hipStream_t s);
// out[r][k] = colscale[k] * (src_row[r] >= 0 ? w[src_row[r]][k] : 0)   (colscale null = 1)
int launch_repack_rows_scaled(const float* w, void* out, const int* src_row_dev, int Npad, int K, const float* colscale,
                              int dtype, hipStream_t s);
// out[n] = sum_k W[n][k] (+ add[n]) over a packed [N][K] matrix in `dtype`, fp32 accumulation
int launch_rowsum(const void* W, const float* add, float* out, int N, int K, int dtype, hipStream_t s);

// Weight formats of the GEMM epilogues, made once here for the handles (engine.hip) and the operator entry points (ops_api.hip).
// Source rows of the packed [2 nout][K] GEGLU projection (EPI_GEGLU): 32-row blocks of 16 value rows | their 16 gate rows, so that
// one lane owns both halves of an output column.  Row r of the packed matrix is row map[r] of ff.net.0.proj ([value | gate]).
std::vector<int> geglu_row_map(int nout);
// dst[0, n) = src (null: nothing), dst[n, Npad) = 0: the bias of a GEMM whose N is padded to its tile
int launch_padded_bias(const float* src, int n, float* dst, int Npad, hipStream_t s);
// A LayerNorm folded into the `parts` Linear layers [Nper][K] behind it, stacked on N (IgemmParams::rowstats / c1):
//   W' = gamma (.) W in the packed row order, c1 = rowsum(W') of the matrix as stored in `dtype`, bias' = W beta + b.
// All pointers are device memory, fp32 unless said otherwise.
struct LnFold {
  int parts = 1;
  const float* w[3] = {};             // [Nper][K] each
  const float* bias[3] = {};          // [Nper] each, or all null
  int Nper = 0, K = 0;
  int Npad = 0;                       // rows of W', c1 and bias' (>= parts * Nper)
  const float* gamma = nullptr;       // [K]
  const float* beta = nullptr;        // [K]
  // packed row -> row of w[0] (-1: a zero row), Npad entries: a one-part fold in another row order (geglu_row_map).  Null: the parts
  // in order and zero rows behind them
  const std::vector<int>* row_map = nullptr;
  // 0: the tensors as they are.  Else W', bias' (not c1's definition) carry this factor: gamma, beta and the biases are scaled by it
  // first (launch_axpby), also where it is 1 - the CLIP encoder's q|k|v has always been built that way
  float scale = 0.f;
  int dtype = DT_BF16;                // of W'
};
size_t ln_fold_scratch_bytes(const LnFold& f);   // build-time scratch of launch_ln_fold (the beta-weighted rows, the row map ...)
// Launches are ordered on `s`; `scratch` may be reused by a later call on the same stream.  W' is [Npad][K] in f.dtype.
int launch_ln_fold(const LnFold& f, void* scratch, void* W, float* c1, float* bias, hipStream_t s);

// CLIP ViT image encoder, row-local kernels (clip_vision.hip)
// image [B,3,H,W] fp32 -> patch-conv GEMM operand [B * (S/P)^2][Kpad], k = (channel, dy, dx), zero padded from 3 P P to Kpad.
// resample = 1: bilinear resize to S x S (align_corners=False, no antialias) and (x - mean[c]) / std[c] first (mean / std: host
// arrays); resample = 0: the image is S x S pixel_values already
int launch_clip_patch_rows(const float* img, void* rows, int B, int H, int W, int S, int P, int Kpad, const float* mean,
                           const float* std, int resample, int dtype, hipStream_t s);
// h[b][t] = LayerNorm((t == 0 ? cls : patch[b][t - 1]) + pos[t]); patch [B][T - 1][C] and h [B][T][C] in the compute dtype
int launch_clip_tokens(const void* patch, const float* cls, const float* pos, const float* gamma, const float* beta, void* h,
                       int B, int T, int C, float eps, int dtype, hipStream_t s);
// out[b] = LayerNorm(h[b][0]) -> fp32 [B][C]
int launch_clip_pooled_ln(const void* h, const float* gamma, const float* beta, float* out, int B, int T, int C, float eps,
                          int dtype, hipStream_t s);
int launch_clip_rows_to_f32(const void* x, float* y, size_t n, int dtype, hipStream_t s);

// CLIP text encoder, row-local kernels (clip_text.hip)
// h[r][t] = tok[ids[r][t]] + pos[t] (fp32 sum, rounded once) -> [R * T][C] in the compute dtype; ids int64 on the device, clamped to
// [0, vocab) for memory safety only
int launch_clip_text_tokens(const int64_t* ids, const float* tok, const float* pos, void* h, int R, int T, int C, int vocab,
                            int dtype, hipStream_t s);
// out[m] = LayerNorm(h[m]) for every row -> fp32 [M][C] (final_layer_norm; two-pass fp32 statistics)
int launch_clip_text_final_ln(const void* h, const float* gamma, const float* beta, float* out, int M, int C, float eps, int dtype,
                              hipStream_t s);

// fp8 (e4m3) operand path of the bf16 attention for the long-context levels (attention_fp8.hip): head dims 40 / 80 only
size_t attention_fp8_scratch_bytes(int B, int N, int C, int heads);
int launch_attention_fp8(const void* qkv, void* kv8_scratch, void* out, int B, int N, int C, int heads, hipStream_t s);
// the same on the 2x-rate block-scaled MFMAs (attention_mx.hip): head dim 40, N a multiple of 128; launch_attention_fp8 routes to it
void attention_mx_set_mode(int m);          // 0: keep attention_fp8.hip's unscaled MFMAs everywhere (A/B)
int attention_mx_get_mode();

// NCHW f32 [B,C,HW] -> NHWC compute dtype [B,HW,Cpad] (zero padded channels), optional affine a*x+b
int launch_pack_nchw(const float* x, void* y, int B, int C, int HW, int Cpad, float mul, float add,
                     int dtype, hipStream_t s);
// three NCHW f32 sources concatenated on channels (torch.cat([latents, rgb, cond],1)); null = skip
int launch_pack_concat3(const float* a, int Ca, const float* b, int Cb, const float* c, int Cc,
                        void* y, int B, int HW, int Cpad, int dtype, hipStream_t s);

// dst = a + b over up to kSkipAddMaxSegs dense tensors of `elems` elements each in one launch (skipadd.hip): the separate image
// encoder's residuals onto the skip connections.  fp32 sum, one rounding to the storage type; dst may be a or b
struct SkipAddSeg { void* dst = nullptr; const void* a = nullptr; const void* b = nullptr; long long elems = 0; };
constexpr int kSkipAddMaxSegs = 12;
int launch_skip_add(const SkipAddSeg* segs, int n_segs, int dtype, hipStream_t s);

// timestep embedding + time MLP + all time_emb_proj: see misc.hip
int launch_time_embed(const int64_t* t_dev, int t_count, int64_t t_host, int B, float* sinus /*[B,320]*/,
                      hipStream_t s);
// y[B][N] = act_in(x[B][K]) @ W[N][K]^T + bias ; f32 small-M GEMV (M<=64)
int launch_small_linear(const float* x, const float* W, const float* bias, float* y, int B, int K, int N,
                        int silu_in, int silu_out, hipStream_t s);

// bilinear x2 (align_corners=False) NHWC compute dtype [B,H,W,C] -> NCHW f32 [B,C,2H,2W]
int launch_bilinear2x_nchw(const void* x, float* y, int B, int H, int W, int C, int dtype, hipStream_t s);

// fused decode tail: bilinear x2 + argmax over C + max-softmax prob; mask_th < 0 disables the threshold
int launch_bilinear2x_argmax(const void* x, int64_t* ids, float* prob, int B, int H, int W, int C, float mask_th,
                             int64_t ignore_label, int dtype, hipStream_t s);

// weight repack (f32 torch layout -> compute dtype [N][K])
// conv OIHW [Co][Ci][kh][kw] -> [Npad][kh*kw][Cipad] ; rows >= Co and channels >= Ci are zero
// cm_tile > 0: channel-major K order [Npad][Cipad / cm_tile][kh*kw][cm_tile] (IgemmParams::cm; cm_tile = K elements per tile)
int launch_repack_conv(const float* w, void* out, int Co, int Ci, int KH, int KW, int Npad, int Cipad,
                       int dtype, hipStream_t s, int cm_tile = 0);
// generic row gather: out[r][:] = (src_row[r] >= 0) ? w[src_row[r]][0:K] : 0  (Linear, GEGLU interleave, qkv concat)
int launch_repack_rows(const float* w, void* out, const int* src_row_dev, int Npad, int K, int dtype, hipStream_t s);
// ConvTranspose2d [Ci][Co][2][2] -> [4*Co][Ci]  (n = (dy*2+dx)*Co + co)
int launch_repack_convt2(const float* w, void* out, int Ci, int Co, int dtype, hipStream_t s);

// DDIM step (ddim_scheduler.py:218-269), elementwise, bit-exact op order
struct DdimCoef { float sqrt_a_t, sqrt_b_t, sqrt_a_prev, sqrt_b_prev; int pred_type; int clip; float clip_range; int use_clipped; };
int launch_ddim_step(const float* eps, const float* x, float* prev, float* x0, size_t n, DdimCoef c, hipStream_t s);
// guided scheduler step (guided.hip): eps [mult*n] (mult 2: uncond | cond halves, combined as uncond + g (cond - uncond), each op
// rounded), DDIM update of latents [n] in place (last: pred_original_sample); cond <- pred_original_sample and lat2 [2n] <- the
// new latents in both halves when non-null
int launch_guided_step(const float* eps, float* latents, float* cond, float* lat2, size_t n, int mult, float g, DdimCoef c,
                       int last, hipStream_t s);
// The tail of a denoising step in one launch (tail.hip, bf16): conv_out on a halo-resident pixel tile and, when ddim != 0,
// the scheduler update, inpainting paste, self-condition write and the next step's packed UNet input in its epilogue.
struct StepTail {
  const void* x = nullptr;        // [B, H*W, 320] SiLU(conv_norm_out(h)), bf16
  const void* w = nullptr;        // conv_out weights packed [N][9*320] bf16 (rows 0..3 real)
  const float* bias = nullptr;
  const void* zeros = nullptr;
  int B = 0, H = 0, W = 0;
  float* eps_out = nullptr;       // [B,4,H,W] fp32: the model output (plain forward); may be null when ddim != 0
  int ddim = 0, last = 0;
  DdimCoef c{};
  float* latents = nullptr;       // [B,4,H,W] fp32, updated in place (last step: pred_original_sample)
  float* cond = nullptr;          // self-condition <- pred_original_sample, or null
  const float* rgb = nullptr;
  void* xin_next = nullptr;       // [B, H*W, 64] bf16: next step's packed input [latents | rgb | cond | 0], or null
  const uint8_t* known = nullptr; const float* z0 = nullptr; const float* noise = nullptr;   // inpainting paste
  float sa = 0.f, sb = 0.f;
};
bool conv_out_tail_ok(int C, int H, int W, int dtype);     // the shape has the kernel and debug key 14 bit 0 allows it
bool step_tail_fused();                                      // key 14 bits 0 and 1: the sampling loop hands the scheduler step to it
void step_tail_set_mode(int m);
int step_tail_get_mode();
int launch_conv_out_tail(const StepTail& t, hipStream_t s);
// out = m ? (sa*z0 + sb*noise) : cur   (inpainting paste; m is u8 [B,1,L,L] broadcast on channels)
int launch_inpaint_paste(float* cur, const float* z0, const float* noise, const uint8_t* known, float sa, float sb,
                         int B, int C, int HW, hipStream_t s);
// add_noise / remove_noise with per-sample timesteps (ddim_scheduler.py:155-216)
int launch_add_noise(const float* x0, const float* noise, const int64_t* t_dev, const float* ac_dev, int n_train, float scale,
                     float* out, int B, size_t per, int remove, hipStream_t s);
// softmax(scale * s) over the last dim of fp32 scores [rows][n] -> probabilities in the compute dtype [rows][n]
int launch_softmax_rows(const float* s, void* p, int rows, int n, float scale, int dtype, hipStream_t st);
int launch_axpby(const float* x, float a, float b, float* y, size_t n, hipStream_t s);  // y = a*x + b
// bit codec of segment ids (ldmseg/data/coco.py:377-390)
int launch_panoptic_postprocess(const float* logits, int B, int C, int HW, int threshold_output, int threshold_mode,
                                float mask_th, int count_th, double overlap_th, int64_t ignore_label, int32_t* labels,
                                int32_t* panoptic, uint8_t* keep, int32_t* counts, int32_t* mask_counts, hipStream_t s);
// fused evaluation tail on the decoder's 4L NHWC output: x2 -> input size -> crop -> original size -> panoptic post-processing
int launch_panoptic_from_decoder(const void* x4, int B, int H4, int W4, int C, int dtype, int in_h, int in_w,
                                 const int32_t* boxes_host, const int32_t* sizes_host, const int64_t* offsets_host,
                                 int threshold_output, int threshold_mode, float mask_th, int count_th, double overlap_th,
                                 int64_t ignore_label, int32_t* labels, int32_t* panoptic, uint8_t* keep, int32_t* counts,
                                 int32_t* mask_counts, hipStream_t s, float* volume = nullptr,    // volume: test hook, [sum_b C * h_b * w_b] fp32
                                 int mask_rule = 0);   // overlap mask: 0 sigmoid(logit) >= mask_th (LDM tail), 1 logit >= mask_th (trainers_ae.py:656)
// SemsegMeter.update (semseg_evaluation.py:24-33): counts int64 [3][K] (tp | fp | fn) += the rule on n (pred, gt) pairs; K <= 256
int launch_semseg_meter(const int64_t* pred, const int64_t* gt, size_t n, int K, int64_t ignore_index, int64_t* counts, hipStream_t s);
// fused mIoU tail on the decoder's 4L NHWC output: align_corners=True bilinear to (oh, ow) -> argmax / max-softmax threshold -> the meter
// rule against targets [B][oh * ow] (trainers_ae.py:754-761); targets / preds / volume (test hook, [B][C][oh * ow] fp32) may be null
int launch_semseg_from_decoder(const void* x4, int B, int H4, int W4, int C, int dtype, int oh, int ow, float mask_th,
                               int64_t ignore_label, const int64_t* targets, int64_t ignore_index, int K, int64_t* preds,
                               int64_t* counts, hipStream_t s, float* volume = nullptr);
// device-side PQ meter (pq_meter.hip): contingency table + IoU > 0.5 matching of a batch of (ground truth, prediction) map pairs;
// arguments as ldmseg_pq_match (include/ldmseg_hip.h)
int launch_pq_match(const int32_t* pred, const void* gt, int gt_format, int B, const int32_t* sizes_host, const int64_t* pred_offsets_host,
                    const int64_t* gt_offsets_host, const uint8_t* keep, int P, const int32_t* gt_counts_host, int Gpad,
                    const int32_t* slot_ids, const uint8_t* slot_crowd, const int64_t* slot_area, const int32_t* slot_meta,
                    int32_t* inter, int32_t* stats, double* match_iou, hipStream_t s);
// the forward half of the training step behind the UNet output (loss.hip); arguments as ldmseg_diffusion_loss (include/ldmseg_hip.h)
struct LossTail {
  const float* pred;          // [B][C][HW] the UNet's output
  const float* target;        // noise or latents; null: no loss (pred_latents only)
  const float* noisy;         // read for pred_type 0 when pred_latents is written
  const int64_t* t;           // [B]
  const float* ac;            // alphas_cumprod [n_train]
  int n_train;
  const float* weights;       // [n_train] or null
  const float* mask;          // [B][HW] or null
  const uint8_t* paste;       // [B][C][HW] or null
  const float* paste_src;
  const float* minmax;        // device {min, max} or null
  float* elem;                // element loss or null
  float* pred_latents;        // or null
  int C, HW;
  int loss_type, pred_type;
  int per;                    // filled by the launcher
  double* partial;
};
size_t diffusion_loss_scratch_bytes(int B, int C, int HW);
// ohem_k: 0 = plain mean; k >= 1 = mean of the k largest element losses (needs elem)
int launch_diffusion_loss(const LossTail& t, int B, double ohem_k, float* sample_sums, float* mean, void* scratch, hipStream_t s);
size_t tensor_minmax_scratch_bytes();
int launch_tensor_minmax(const float* x, size_t n, float* out, void* scratch, hipStream_t s);
int launch_loss_weight_mask(const void* src, int src_dtype, int B, int Hi, int Wi, int h, int w, int mode, int64_t ignore_label,
                            float* out, int32_t* flag, hipStream_t s);
// the seg-VAE's stage-1 loss (point_loss.hip); arguments as ldmseg_point_loss / ldmseg_class_presence / ldmseg_gaussian_kl
// (include/ldmseg_hip.h)
struct PointLoss {
  const float* x;             // [B][C][H][W] logits
  int B, C, H, W;
  const int64_t* tgt;         // [B][Ht][Wt]
  const uint8_t* valid;       // [B][Ht][Wt] or null
  int Ht, Wt;
  const int32_t* rows;        // [N] b * C + c of the mask rows, by image, then class id
  int N;
  const float* ce_over;       // [B][S][2] or null (S == 0)
  const float* ce_fresh;      // [B][P - kU][2] or null (P == kU)
  const float* m_over;        // [N][S][2]
  const float* m_fresh;       // [N][P - kU][2]
  int S, kU, P;
  int64_t ignore;
  float temperature;
  float* unc;                 // filled by the launcher
  int32_t* sel;
  double* partial;
};
int launch_class_presence(const int64_t* targets, const uint8_t* valid, int B, int Ht, int Wt, int C, int64_t ignore_label,
                          uint8_t* present, int32_t* flag, hipStream_t s);
size_t point_loss_scratch_bytes(int rows, int S, int kU, int P);
int launch_point_loss(const PointLoss& p, double num_masks, float* out, int32_t* selected, void* scratch, hipStream_t s);
int launch_gaussian_kl(const float* moments, int B, int n, float* per_image, float* mean, hipStream_t s);
// its backward to the logits and to the moments (point_loss_bwd.hip); arguments as ldmseg_point_loss_backward /
// ldmseg_gaussian_kl_backward
struct PointLossGrad {
  PointLoss f;                // the forward's arguments; f.sel = the forward's `selected`
  double num_masks;
  const float* g_ce;          // device scalars d(result) / d(ce), d(result) / d(mask); null: that term's rows take no part
  const float* g_mask;
  float* grad_x;              // [B][C][H][W], every element written
  double* stat;               // filled by the launcher
  float* rec_a;
  float* rec_b;
  int32_t* rec_label;
  int32_t* count;
  int32_t* cursor;
  int32_t* img_base;
  unsigned long long* entries;
};
size_t point_loss_backward_scratch_bytes(int B, int C, int H, int W, int N, int kU, int P);
int launch_point_loss_backward(const PointLossGrad& g, void* scratch, hipStream_t s);
int launch_gaussian_kl_backward(const float* moments, int B, int n, const float* grad_per_image, float* grad_moments, hipStream_t s);
int launch_bit_encode(const int64_t* ids, float* out, uint8_t* ignore, int B, int n, int HW, int64_t ignore_label,
                      float fill, float mul, float add, hipStream_t s);
int launch_bit_decode(const float* x, int64_t* out, int B, int n, int HW, hipStream_t s);
// mean + exp(0.5*clamp(logvar))*noise on NCHW moments [B,8,HW] -> [B,4,HW]
int launch_posterior_sample(const float* moments, const float* noise, float* out, int B, int HW, hipStream_t s);

}  // namespace ldmseg
