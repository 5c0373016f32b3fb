// The single definitions behind runtime.h, and the part of the C ABI (include/ldmseg_hip.h) that drives no model handle: the
// profiler, the scheduler and loss operators, the bit codec, the evaluation meters, ldmseg_last_error / ldmseg_version.
#include <cstdio>
#include <cstring>

#include "runtime.h"

namespace ldmseg::rt {

thread_local std::string g_err;
int g_plan_epoch = 0;
int g_gnfold_mode = 1, g_sepenc_every_step = 0, g_ffp_mode = 1;      // debug keys 22, 25, 20: the table of debug_knobs.hip says what they mean
Profiler g_prof;

int alloc_gn_sync(void** out) {
  void* p = nullptr;
  if (hipMalloc(&p, gn_sync_bytes()) != hipSuccess) return fail(LDMSEG_E_OOM, "hipMalloc of the GroupNorm hand-off region failed");
  if (gn_sync_init(p, nullptr) != 0 || hipStreamSynchronize(nullptr) != hipSuccess) { (void)hipFree(p); return fail(LDMSEG_E_HIP, "GroupNorm hand-off region init failed"); }
  *out = p;
  return 0;
}
int alloc_cf_sync(void** out) {
  void* p = nullptr;
  if (hipMalloc(&p, igemm_cf_bytes()) != hipSuccess) return fail(LDMSEG_E_OOM, "hipMalloc of the split-K counter region failed");
  if (hipMemset(p, 0, igemm_cf_bytes()) != hipSuccess) { (void)hipFree(p); return fail(LDMSEG_E_HIP, "split-K counter region init failed"); }
  *out = p;
  return 0;
}

Exec make_exec(HandleBase& h, int B, hipStream_t s, bool dry, size_t scratch_base) {
  h.ws.begin(dry, scratch_base);
  Exec ex{&h.ws, h.dt, B, s};
  ex.gn_sync = h.gn_sync;
  ex.cf_sync = h.cf_sync;
  ex.x3 = h.x3 ? 2 : 0;          // (2: the handle's weights are hi | lo planes, Builder::finish)
  return ex;
}

int build_resnet(Builder& b, const std::string& p, int cin, int cout, int* temb_off, ResnetW* r) {
  r->cin = cin; r->cout = cout;
  TRY(b.norm(p + "norm1", cin, &r->norm1));
  // (the 320- / 640-channel levels can run on maps of 64x64 and more: they also hold the channel-major packing, see igemm_conv_cm)
  TRY(b.conv(p + "conv1", cout, cin, 3, cin, &r->conv1, true, 0, EPI_STORE, cout <= 640));
  TRY(b.norm(p + "norm2", cout, &r->norm2));
  TRY(b.conv(p + "conv2", cout, cout, 3, cout, &r->conv2, true, 0, EPI_STORE, cout <= 640));
  r->has_shortcut = cin != cout;
  if (r->has_shortcut) TRY(b.conv(p + "conv_shortcut", cout, cin, 1, cin, &r->shortcut));
  // conv2(h) + conv_shortcut(x) is one accumulation over K = 9 cout + cin: a second packing with the shortcut's columns behind
  // conv2's, run as one launch with an extra centre tap (igemm.hip, XT) - the shortcut's own launch, its output tensor and the
  // residual read of conv2's epilogue disappear (14 resnets of the UNet)
  if (r->has_shortcut && b.dt == DT_BF16 && r->conv2.N == r->shortcut.N && r->conv2.N % 160 == 0 && cin % bke(b.dt) == 0 && cout % bke(b.dt) == 0) {
    ConvW& x = r->conv2x;
    x.N = r->conv2.N; x.n_valid = r->conv2.n_valid; x.cin_pad = cout; x.taps = 9; x.cout = cout; x.xt_cin = cin;
    TRY(b.arena->alloc(&x.w, (size_t)x.N * (9 * cout + cin) * esize(b.dt)));
    TRY(launch_concat_rows(r->conv2.w, 9 * cout, r->shortcut.w, cin, x.w, x.N, b.dt, b.s));
    void* pb;
    TRY(b.arena->alloc(&pb, x.N * sizeof(float)));
    x.bias = (float*)pb;
    TRY(launch_vec_add(r->conv2.bias, r->shortcut.bias, x.bias, x.N, b.s));
  }
  r->temb_off = *temb_off;
  *temb_off += cout;
  return 0;
}

int ensure_ws(HandleBase& h, size_t need) {
  if (need <= h.ws_cap) return 0;
  if (h.ws_mem) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipFree(h.ws_mem));
    h.ws_mem = nullptr;
    h.ws_cap = 0;
  }
  if (hipMalloc(&h.ws_mem, need) != hipSuccess) return fail(LDMSEG_E_OOM, "workspace hipMalloc failed (" + std::to_string(need) + " bytes)");
  h.ws_cap = need;
  h.ws.base = (char*)h.ws_mem;
  h.ws.cap = need;
  return 0;
}

int check_arch(int device) {
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(LDMSEG_E_ARCH, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
  return 0;
}

int make_weight_map(int n, const char* const* names, const void* const* ptrs, const int64_t* numels, WeightMap* wm) {
  if (!names || !ptrs || !numels) return fail(LDMSEG_E_ARG, "null weight arrays");
  for (int i = 0; i < n; ++i) wm->m[names[i]] = {(const float*)ptrs[i], numels[i]};
  return 0;
}

}  // namespace ldmseg::rt

using namespace ldmseg;
using namespace ldmseg::rt;

extern "C" {

const char* ldmseg_last_error(void) { return g_err.c_str(); }
const char* ldmseg_version(void) { return "ldmseg_hip 0.1 (gfx950)"; }

int ldmseg_semseg_meter_update(const int64_t* pred, const int64_t* gt, int64_t n, int num_classes, int64_t ignore_index,
                               int64_t* counts, void* stream) {
  g_err.clear();
  if (!counts || n < 0 || (n > 0 && (!pred || !gt))) return fail(LDMSEG_E_ARG, "null argument");
  if (num_classes < 1 || num_classes > 256) return fail(LDMSEG_E_ARG, "num_classes must be 1..256");
  TRY(launch_semseg_meter(pred, gt, (size_t)n, num_classes, ignore_index, counts, (hipStream_t)stream));
  return 0;
}

int ldmseg_pq_match(const int32_t* pred, const void* gt, int gt_format, int B, const int32_t* sizes, const int64_t* pred_offsets,
                    const int64_t* gt_offsets, const uint8_t* keep, int P, const int32_t* gt_counts, int Gpad,
                    const int32_t* slot_ids, const uint8_t* slot_crowd, const int64_t* slot_area, const int32_t* slot_meta,
                    int32_t* inter, int32_t* stats, double* match_iou, void* stream) {
  g_err.clear();
  if (!pred || !gt || !sizes || !pred_offsets || !gt_offsets || !keep || !gt_counts || !slot_ids || !slot_crowd || !slot_area ||
      !slot_meta || !inter || !stats || !match_iou)
    return fail(LDMSEG_E_ARG, "null argument");
  if (B < 1 || P < 1 || P > 256) return fail(LDMSEG_E_ARG, "B >= 1 and P in 1..256");
  if (Gpad < 1 || Gpad > LDMSEG_PQ_G_MAX) return fail(LDMSEG_E_ARG, "Gpad must be 1..LDMSEG_PQ_G_MAX");
  if (gt_format != 0 && gt_format != 1) return fail(LDMSEG_E_ARG, "gt_format: 0 int32 ids, 1 uint8 RGB");
  for (int b = 0; b < B; ++b)
    if (gt_counts[b] < 0 || gt_counts[b] > Gpad || sizes[2 * b] < 1 || sizes[2 * b + 1] < 1 ||
        (int64_t)sizes[2 * b] * sizes[2 * b + 1] > (int64_t)0x7fff0000 || pred_offsets[b] < 0 || gt_offsets[b] < 0)
      return fail(LDMSEG_E_SHAPE, "bad size / offset / declared count of image " + std::to_string(b));
  TRY(launch_pq_match(pred, gt, gt_format, B, sizes, pred_offsets, gt_offsets, keep, P, gt_counts, Gpad, slot_ids, slot_crowd,
                      slot_area, slot_meta, inter, stats, match_iou, (hipStream_t)stream));
  return 0;
}

int ldmseg_vae_posterior(const float* moments, const float* noise, float out_scale, int B, int l, float* out,
                         void* stream) {
  g_err.clear();
  if (!moments || !out) return fail(LDMSEG_E_ARG, "null argument");
  TRY(launch_posterior_sample(moments, noise, out, B, l * l, (hipStream_t)stream));
  if (out_scale != 1.0f) TRY(launch_axpby(out, out_scale, 0.f, out, (size_t)B * 4 * l * l, (hipStream_t)stream));
  return 0;
}

int ldmseg_ddim_step(const float* model_output, const float* sample, float sqrt_alpha_t, float sqrt_beta_t,
                     float sqrt_alpha_prev, float sqrt_beta_prev, int prediction_type, int clip_sample,
                     float clip_sample_range, int use_clipped_model_output, float* prev_sample,
                     float* pred_original_sample, size_t n, void* stream) {
  g_err.clear();
  if (!model_output || !sample) return fail(LDMSEG_E_ARG, "null argument");
  if (prediction_type < 0 || prediction_type > 2) return fail(LDMSEG_E_ARG, "unknown prediction_type");
  DdimCoef c{sqrt_alpha_t, sqrt_beta_t, sqrt_alpha_prev, sqrt_beta_prev, prediction_type, clip_sample, clip_sample_range,
             use_clipped_model_output};
  TRY(launch_ddim_step(model_output, sample, prev_sample, pred_original_sample, n, c, (hipStream_t)stream));
  return 0;
}

// add_noise (remove = 0) and its inverse, one launcher: the checks and the launch both entries share
static int noise_entry(const float* x, const float* noise, const int64_t* t, const float* ac, int n_train, float scale, float* out, int B, size_t per,
                       int remove, void* stream) {
  g_err.clear();
  if (!x || !noise || !t || !ac || !out) return fail(LDMSEG_E_ARG, "null argument");
  if (B < 1 || per < 1 || n_train < 1) return fail(LDMSEG_E_ARG, "B, per_sample and n_train_timesteps must be positive");
  TRY(launch_add_noise(x, noise, t, ac, n_train, scale, out, B, per, remove, (hipStream_t)stream));
  return 0;
}
int ldmseg_add_noise(const float* original, const float* noise, const int64_t* timesteps_dev, const float* alphas_cumprod_dev,
                     int n_train_timesteps, float scale, float* out, int B, size_t per_sample, void* stream) {
  return noise_entry(original, noise, timesteps_dev, alphas_cumprod_dev, n_train_timesteps, scale, out, B, per_sample, 0, stream);
}
int ldmseg_remove_noise(const float* noisy, const float* noise, const int64_t* timesteps_dev, const float* alphas_cumprod_dev,
                        int n_train_timesteps, float scale, float* out, int B, size_t per_sample, void* stream) {
  return noise_entry(noisy, noise, timesteps_dev, alphas_cumprod_dev, n_train_timesteps, scale, out, B, per_sample, 1, stream);
}

size_t ldmseg_diffusion_loss_scratch_bytes(int B, int C, int HW) { return diffusion_loss_scratch_bytes(B, C, HW); }

int ldmseg_diffusion_loss(const float* prediction, const float* target, const float* noisy, const int64_t* timesteps_dev,
                          const float* alphas_cumprod_dev, int n_train_timesteps, const float* weights_dev,
                          const float* loss_mask, const uint8_t* paste_mask, const float* paste_src, const float* minmax_dev,
                          int loss_type, int prediction_type, double ohem_ratio, int B, int C, int HW, float* elem_loss,
                          float* pred_latents, float* mean, float* sample_sums, void* scratch, void* stream) {
  g_err.clear();
  if (!prediction || !timesteps_dev || !alphas_cumprod_dev || !scratch) return fail(LDMSEG_E_ARG, "null argument");
  if (!target && !pred_latents) return fail(LDMSEG_E_ARG, "nothing to compute: neither a target nor pred_latents");
  if (target && !mean) return fail(LDMSEG_E_ARG, "a loss needs the mean output");
  if (B < 1 || B > 65535 || C < 1 || HW < 1 || n_train_timesteps < 1 || (int64_t)C * HW > (int64_t)0x7fff0000)
    return fail(LDMSEG_E_SHAPE, "B in 1..65535, C, HW and n_train_timesteps positive, C * HW < 2^31");
  if (loss_type != LDMSEG_LOSS_L1 && loss_type != LDMSEG_LOSS_L2 && loss_type != LDMSEG_LOSS_SMOOTH_L1)
    return fail(LDMSEG_E_ARG, "unknown loss_type");
  if (prediction_type != 0 && prediction_type != 1) return fail(LDMSEG_E_ARG, "prediction_type: 0 epsilon, 1 sample");
  if (pred_latents && prediction_type == 0 && !noisy) return fail(LDMSEG_E_ARG, "epsilon pred_latents need the noisy latents");
  if ((paste_mask != nullptr) != (paste_src != nullptr)) return fail(LDMSEG_E_ARG, "paste_mask and paste_src come together");
  double k = 0;
  if (target && ohem_ratio < 1.0) {
    if (!elem_loss) return fail(LDMSEG_E_ARG, "ohem_ratio < 1 needs the elem_loss buffer");
    k = (double)(int64_t)(ohem_ratio * (double)((int64_t)B * C * HW));
    if (!(k >= 1)) return fail(LDMSEG_E_ARG, "ohem_ratio selects no element (k == 0)");
  }
  LossTail t{};
  t.pred = prediction; t.target = target; t.noisy = noisy; t.t = timesteps_dev; t.ac = alphas_cumprod_dev;
  t.n_train = n_train_timesteps; t.weights = weights_dev; t.mask = loss_mask; t.paste = paste_mask; t.paste_src = paste_src;
  t.minmax = minmax_dev; t.elem = elem_loss; t.pred_latents = pred_latents; t.C = C; t.HW = HW;
  t.loss_type = loss_type; t.pred_type = prediction_type;
  TRY(launch_diffusion_loss(t, B, k, sample_sums, mean, scratch, (hipStream_t)stream));
  return 0;
}

int ldmseg_loss_weight_mask(const void* src, int src_dtype, int B, int Hi, int Wi, int h, int w, int mode, int64_t ignore_label,
                            float* out, int32_t* flag, void* stream) {
  g_err.clear();
  if (!src || !out || !flag) return fail(LDMSEG_E_ARG, "null argument");
  if (src_dtype < 0 || src_dtype > 2) return fail(LDMSEG_E_ARG, "src_dtype: 0 int64, 1 uint8, 2 fp32");
  if (mode != LDMSEG_MASK_IGNORE && mode != LDMSEG_MASK_PADDING && mode != LDMSEG_MASK_COUNTS) return fail(LDMSEG_E_ARG, "unknown mode");
  if (B < 1 || Hi < 1 || Wi < 1 || h < 1 || w < 1 || (int64_t)h * w > (int64_t)0x7fff0000) return fail(LDMSEG_E_SHAPE, "sizes must be positive");
  TRY(launch_loss_weight_mask(src, src_dtype, B, Hi, Wi, h, w, mode, ignore_label, out, flag, (hipStream_t)stream));
  return 0;
}

int ldmseg_tensor_minmax(const float* x, size_t n, float* minmax, void* scratch, void* stream) {
  g_err.clear();
  static_assert(LDMSEG_MINMAX_SCRATCH_BYTES == 256 * 3 * sizeof(float), "header and kernel disagree on the partials");
  if (!x || !minmax || !scratch) return fail(LDMSEG_E_ARG, "null argument");
  if (n < 1) return fail(LDMSEG_E_ARG, "min / max of an empty tensor");
  if (tensor_minmax_scratch_bytes() > (size_t)LDMSEG_MINMAX_SCRATCH_BYTES) return fail(LDMSEG_E_ARG, "scratch size mismatch");
  TRY(launch_tensor_minmax(x, n, minmax, scratch, (hipStream_t)stream));
  return 0;
}

size_t ldmseg_point_loss_scratch_bytes(int rows, int S, int kU, int P) { return point_loss_scratch_bytes(rows, S, kU, P); }

int ldmseg_class_presence(const int64_t* targets, const uint8_t* valid, int B, int Ht, int Wt, int C, int64_t ignore_label,
                          uint8_t* present, int32_t* flag, void* stream) {
  g_err.clear();
  if (!targets || !present || !flag) return fail(LDMSEG_E_ARG, "null argument");
  if (B < 1 || B > 65535 || Ht < 1 || Wt < 1 || (int64_t)Ht * Wt > (int64_t)0x7fff0000) return fail(LDMSEG_E_SHAPE, "B in 1..65535, Ht * Wt in 1..2^31");
  if (C < 1 || C > LDMSEG_POINT_LOSS_MAX_C) return fail(LDMSEG_E_SHAPE, "C must be 1..LDMSEG_POINT_LOSS_MAX_C");
  TRY(launch_class_presence(targets, valid, B, Ht, Wt, C, ignore_label, present, flag, (hipStream_t)stream));
  return 0;
}

int ldmseg_point_loss(const float* x, int B, int C, int H, int W, const int64_t* targets, const uint8_t* valid, int Ht, int Wt,
                      const int32_t* mask_rows_dev, int N, const float* ce_over, const float* ce_fresh, const float* mask_over,
                      const float* mask_fresh, int S, int kU, int P, int64_t ignore_label, float temperature, double num_masks,
                      float* out, int32_t* selected, void* scratch, void* stream) {
  g_err.clear();
  if (!x || !targets || !out || !scratch) return fail(LDMSEG_E_ARG, "null argument");
  if (C < 1 || C > LDMSEG_POINT_LOSS_MAX_C) return fail(LDMSEG_E_SHAPE, "C must be 1..LDMSEG_POINT_LOSS_MAX_C");
  if (B < 1 || N < 0 || N > B * C || B + N > 65535) return fail(LDMSEG_E_SHAPE, "B >= 1, 0 <= N <= B * C, B + N <= 65535");
  if (H < 1 || W < 1 || Ht < 1 || Wt < 1 || (int64_t)H * W > (int64_t)0x7fff0000 || (int64_t)Ht * Wt > (int64_t)0x7fff0000)
    return fail(LDMSEG_E_SHAPE, "map sizes must be positive, H * W and Ht * Wt below 2^31");
  if (P < 1 || kU < 0 || kU > P || S < kU || (kU > 0 && S < 1) || (int64_t)(B + N) * (S > P ? S : P) > (int64_t)0x3fff0000)
    return fail(LDMSEG_E_ARG, "need 0 <= kU <= P, kU <= S, (B + N) * max(S, P) below 2^30");
  if (!(temperature > 0.0f)) return fail(LDMSEG_E_ARG, "temperature must be positive");
  if (N > 0 && (!mask_rows_dev || !(num_masks > 0.0))) return fail(LDMSEG_E_ARG, "mask rows need mask_rows_dev and num_masks > 0");
  if (kU > 0 && (!ce_over || (N > 0 && !mask_over))) return fail(LDMSEG_E_ARG, "kU > 0 needs the oversampled draws");
  if (P > kU && (!ce_fresh || (N > 0 && !mask_fresh))) return fail(LDMSEG_E_ARG, "P > kU needs the fresh draws");
  PointLoss p{};
  p.x = x; p.B = B; p.C = C; p.H = H; p.W = W; p.tgt = targets; p.valid = valid; p.Ht = Ht; p.Wt = Wt;
  p.rows = mask_rows_dev; p.N = N; p.ce_over = ce_over; p.ce_fresh = ce_fresh; p.m_over = mask_over; p.m_fresh = mask_fresh;
  p.S = S; p.kU = kU; p.P = P; p.ignore = ignore_label; p.temperature = temperature;
  TRY(launch_point_loss(p, num_masks, out, selected, scratch, (hipStream_t)stream));
  return 0;
}

int ldmseg_gaussian_kl(const float* moments, int B, int latent_channels, int HW, float* per_image, float* mean, void* stream) {
  g_err.clear();
  if (!moments || !per_image) return fail(LDMSEG_E_ARG, "null argument");
  if (B < 1 || B > 65535 || latent_channels < 1 || HW < 1 || (int64_t)latent_channels * HW > (int64_t)0x3fff0000)
    return fail(LDMSEG_E_SHAPE, "B in 1..65535, latent_channels * HW in 1..2^30");
  TRY(launch_gaussian_kl(moments, B, latent_channels * HW, per_image, mean, (hipStream_t)stream));
  return 0;
}

size_t ldmseg_point_loss_backward_scratch_bytes(int B, int C, int H, int W, int N, int kU, int P) {
  if (C > LDMSEG_POINT_LOSS_MAX_C) return 0;
  return point_loss_backward_scratch_bytes(B, C, H, W, N, kU, P);
}

int ldmseg_point_loss_backward(const float* x, int B, int C, int H, int W, const int64_t* targets, const uint8_t* valid, int Ht,
                               int Wt, const int32_t* mask_rows_dev, int N, const float* ce_over, const float* ce_fresh,
                               const float* mask_over, const float* mask_fresh, const int32_t* selected, int S, int kU, int P,
                               int64_t ignore_label, float temperature, double num_masks, const float* grad_ce_dev,
                               const float* grad_mask_dev, float* grad_x, void* scratch, void* stream) {
  g_err.clear();
  if (!x || !targets || !grad_x || !scratch) return fail(LDMSEG_E_ARG, "null argument");
  if (C < 1 || C > LDMSEG_POINT_LOSS_MAX_C) return fail(LDMSEG_E_SHAPE, "C must be 1..LDMSEG_POINT_LOSS_MAX_C");
  if (B < 1 || N < 0 || N > B * C || B + N > 65535) return fail(LDMSEG_E_SHAPE, "B >= 1, 0 <= N <= B * C, B + N <= 65535");
  if (H < 1 || W < 1 || Ht < 1 || Wt < 1 || (int64_t)H * W > (int64_t)0x7fff0000 || (int64_t)Ht * Wt > (int64_t)0x7fff0000)
    return fail(LDMSEG_E_SHAPE, "map sizes must be positive, H * W and Ht * Wt below 2^31");
  if (P < 1 || kU < 0 || kU > P || S < kU || (kU > 0 && S < 1) || (int64_t)(B + N) * (S > P ? S : P) > (int64_t)0x1fff0000)
    return fail(LDMSEG_E_ARG, "need 0 <= kU <= P, kU <= S, (B + N) * max(S, P) below 2^29");
  if (!(temperature > 0.0f)) return fail(LDMSEG_E_ARG, "temperature must be positive");
  if (N > 0 && (!mask_rows_dev || !(num_masks > 0.0))) return fail(LDMSEG_E_ARG, "mask rows need mask_rows_dev and num_masks > 0");
  if (kU > 0 && (!selected || !ce_over || (N > 0 && !mask_over)))
    return fail(LDMSEG_E_ARG, "kU > 0 needs the oversampled draws and the forward's selected indices");
  if (P > kU && (!ce_fresh || (N > 0 && !mask_fresh))) return fail(LDMSEG_E_ARG, "P > kU needs the fresh draws");
  PointLossGrad g{};
  PointLoss& p = g.f;
  p.x = x; p.B = B; p.C = C; p.H = H; p.W = W; p.tgt = targets; p.valid = valid; p.Ht = Ht; p.Wt = Wt;
  p.rows = mask_rows_dev; p.N = N; p.ce_over = ce_over; p.ce_fresh = ce_fresh; p.m_over = mask_over; p.m_fresh = mask_fresh;
  p.S = S; p.kU = kU; p.P = P; p.ignore = ignore_label; p.temperature = temperature;
  p.sel = const_cast<int32_t*>(selected);            // (read only)
  g.num_masks = N > 0 ? num_masks : 1.0;
  g.g_ce = grad_ce_dev; g.g_mask = N > 0 ? grad_mask_dev : nullptr; g.grad_x = grad_x;
  TRY(launch_point_loss_backward(g, scratch, (hipStream_t)stream));
  return 0;
}

int ldmseg_gaussian_kl_backward(const float* moments, int B, int latent_channels, int HW, const float* grad_per_image_dev,
                                float* grad_moments, void* stream) {
  g_err.clear();
  if (!moments || !grad_per_image_dev || !grad_moments) return fail(LDMSEG_E_ARG, "null argument");
  if (B < 1 || B > 65535 || latent_channels < 1 || HW < 1 || (int64_t)latent_channels * HW > (int64_t)0x3fff0000)
    return fail(LDMSEG_E_SHAPE, "B in 1..65535, latent_channels * HW in 1..2^30");
  TRY(launch_gaussian_kl_backward(moments, B, latent_channels * HW, grad_per_image_dev, grad_moments, (hipStream_t)stream));
  return 0;
}

int ldmseg_bit_encode(const int64_t* ids, int B, int n_bits, int HW, int64_t ignore_label, float fill_value, float mul,
                      float add, float* bits, uint8_t* ignore_mask, void* stream) {
  g_err.clear();
  if (!ids || !bits || n_bits < 1 || n_bits > 31) return fail(LDMSEG_E_ARG, "bad bit_encode argument");
  TRY(launch_bit_encode(ids, bits, ignore_mask, B, n_bits, HW, ignore_label, fill_value, mul, add, (hipStream_t)stream));
  return 0;
}
int ldmseg_bit_decode(const float* x, int B, int n_bits, int HW, int64_t* ids, void* stream) {
  g_err.clear();
  if (!x || !ids || n_bits < 1 || n_bits > 24) return fail(LDMSEG_E_ARG, "bad bit_decode argument");
  TRY(launch_bit_decode(x, ids, B, n_bits, HW, (hipStream_t)stream));
  return 0;
}

int ldmseg_panoptic_postprocess(const float* logits, int B, int C, int H, int W, int threshold_output, int threshold_mode,
                                float mask_th, int count_th, double overlap_th, int64_t ignore_label, int32_t* labels,
                                int32_t* panoptic, uint8_t* keep, int32_t* counts, int32_t* mask_counts, void* stream) {
  g_err.clear();
  if (!logits || !labels || !panoptic || !keep || !counts || !mask_counts || B < 1 || C < 1 || C > 256 || H < 1 || W < 1 ||
      (threshold_mode != 0 && threshold_mode != 1))
    return fail(LDMSEG_E_ARG, "bad panoptic_postprocess argument");
  TRY(launch_panoptic_postprocess(logits, B, C, H * W, threshold_output, threshold_mode, mask_th, count_th, overlap_th,
                                  ignore_label, labels, panoptic, keep, counts, mask_counts, (hipStream_t)stream));
  return 0;
}

int ldmseg_profile_enable(int enable) { g_prof.on = enable != 0; return 0; }
int ldmseg_profile_reset(void) {
  for (auto& f : g_prof.fam) {
    for (auto& e : f.ev) { g_prof.pool.push_back(e.first); g_prof.pool.push_back(e.second); }
    f.ev.clear();
    f.label.clear();
    f.lflops.clear();
    f.launches = 0;
    f.flops = f.bytes = 0;
  }
  return 0;
}
int ldmseg_profile_read(int family, int64_t* launches, double* total_ms, double* flops, double* bytes) {
  g_err.clear();
  if (family < 0 || family > 4) return fail(LDMSEG_E_ARG, "family must be 0..4");
  ProfFamily& f = g_prof.fam[family];
  double ms = 0;
  for (auto& e : f.ev) {
    HIP_TRY(hipEventSynchronize(e.second));
    float t = 0;
    HIP_TRY(hipEventElapsedTime(&t, e.first, e.second));
    ms += t;
  }
  if (launches) *launches = f.launches;
  if (total_ms) *total_ms = ms;
  if (flops) *flops = f.flops;
  if (bytes) *bytes = f.bytes;
  return 0;
}

// one CSV line per recorded launch: family,label,ms,flops
int ldmseg_profile_dump(const char* path) {
  g_err.clear();
  FILE* fp = std::fopen(path, "w");
  if (!fp) return fail(LDMSEG_E_ARG, "cannot open profile dump file");
  std::fprintf(fp, "family,label,ms,flops\n");
  for (int fi = 0; fi < 5; ++fi) {
    ProfFamily& f = g_prof.fam[fi];
    for (size_t i = 0; i < f.ev.size(); ++i) {
      (void)hipEventSynchronize(f.ev[i].second);
      float t = 0;
      (void)hipEventElapsedTime(&t, f.ev[i].first, f.ev[i].second);
      std::fprintf(fp, "%d,%s,%.6f,%.0f\n", fi, i < f.label.size() ? f.label[i].c_str() : "", t,
                   i < f.lflops.size() ? f.lflops[i] : 0.0);
    }
  }
  std::fclose(fp);
  return 0;
}

}  // extern "C"
