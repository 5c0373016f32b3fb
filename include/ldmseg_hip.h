/* ldmseg_hip.h - C ABI of libldmseg_hip.so, the MI355X (gfx950) implementation of
 * the LDMSeg denoising path.
 *
 * The reference (segments-ai/latent-diffusion-segmentation) has no FFI layer: the
 * seam is the Python call surface TrainerDiffusion uses.  Each entry point below
 * names the reference interface it stands behind (paths relative to the
 * reference root); INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *   - every pointer named *dev* / tensor argument is a DEVICE pointer on the
 *     handle's GPU; boundary tensors are fp32 NCHW contiguous (the reference's
 *     layout); timesteps are int64.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls
 *     only enqueue work.  The one exception is workspace growth: the first call of a
 *     handle at a (B, L) larger than any before (re)allocates its workspace, which
 *     synchronises the device.  ldmseg_unet_reserve() does that up front (workspace,
 *     sampler buffers incl. the time-embedding table of up to 64 steps, the
 *     per-device zero page; the GroupNorm hand-off region belongs to the handle and
 *     is made at *_create), after which forward / sample_loop calls at that size
 *     never allocate or synchronise.  The first launch of each kernel instantiation
 *     in a process still sets a function attribute (host-side, no device work): run
 *     one warm-up forward before capturing a stream.  ldmseg_unet_forward with a
 *     device timestep (t_dev) may be captured into a HIP graph and replayed (the
 *     cooperative GroupNorm draws its hand-off generation on the device, so replays
 *     do not meet each other's records); ldmseg_sample_loop copies cfg->timesteps
 *     from pageable host memory on every call and is not meant to be captured.
 *     *_create calls allocate and synchronise.
 *   - return 0 on success, negative LDMSEG_E_* on failure; ldmseg_last_error()
 *     returns a thread-local message.  No C++ exception crosses the boundary.
 *   - the library owns handles, repacked weights and workspaces; the caller owns
 *     every tensor it passes and keeps it alive until the stream work is done.
 *     Weights are copied/repacked at create time.
 *   - a handle is bound to cfg.device and is not thread-safe (one process per GPU,
 *     like tools/main_ldm.py:69 mp.spawn).  Every call on a handle makes that device
 *     current for its duration and restores the caller's; the handle-free calls
 *     (ddim_step, add_noise, ...) run on the calling thread's current device.
 */
#ifndef LDMSEG_HIP_H_
#define LDMSEG_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LDMSEG_OK 0
#define LDMSEG_E_ARG (-1)      /* bad argument / unsupported option */
#define LDMSEG_E_SHAPE (-2)    /* shape not supported by the kernels */
#define LDMSEG_E_HIP (-3)      /* HIP runtime error (message has the hipError string) */
#define LDMSEG_E_WEIGHT (-4)   /* missing / mis-sized state-dict entry */
#define LDMSEG_E_ARCH (-5)     /* device is not gfx950 */
#define LDMSEG_E_OOM (-6)

#define LDMSEG_F32 0           /* fp32 storage, exact-f32 MFMA: the parity mode (1e-3 vs torch-CPU) */
#define LDMSEG_BF16 1          /* bf16 storage + bf16 MFMA, fp32 accumulate/statistics: the perf mode */
#define LDMSEG_BF16X3 2        /* fp32 storage, norms / softmax / scheduler in fp32, GEMM and attention products on the bf16 MFMAs as hi + lo
                                * (three MFMAs per product block, fp32 accumulation; relative error per product < 2^-16):
                                * the parity-grade throughput mode - inside the 1e-3 bound at several times the exact mode's speed */

#define LDMSEG_PRED_EPSILON 0
#define LDMSEG_PRED_SAMPLE 1
#define LDMSEG_PRED_V 2

typedef struct ldmseg_unet ldmseg_unet;  /* opaque */
typedef struct ldmseg_vae ldmseg_vae;    /* opaque */
typedef struct ldmseg_vae_image ldmseg_vae_image;  /* opaque */

/* ---- UNet: ldmseg/models/unet.py::UNet (UNet2DConditionModel, SD-1.x topology) ---------- */
typedef struct {
  int32_t in_channels;      /* 8 | 12 after UNet.modify_encoder (unet.py:178-233); 4 = vanilla */
  int32_t cross_attention;  /* 0: attn2/norm2 removed (unet.py:83-105, base.yaml:71).  1: every transformer block runs
                             * h = attn2(norm2(h), ctx) + h after attn1 (image_descriptors none / clip_image / clip_image_proj):
                             * the state dict must hold norm2 and attn2.{to_q, to_k, to_v, to_out.0} of all 16 transformers
                             * (cross_attention_dim 768) and may hold encoder_hid_proj.{weight, bias} [768, 1024]; such a handle
                             * runs through ldmseg_unet_forward_ctx / ldmseg_sample_loop_guided only */
  int32_t compute_dtype;    /* LDMSEG_F32 | LDMSEG_BF16 | LDMSEG_BF16X3 */
  int32_t device;           /* HIP device ordinal */
} ldmseg_unet_cfg;

/* Build a UNet from a state dict in the reference's key layout (the `unet` entry of
 * ldmseg.pt, trainers_ldm_cond.py:1791-1814; keys = SURVEY.md App. A).  `names[i]` is
 * the key, `dev_ptrs[i]` an fp32 device tensor in torch layout with `numels[i]`
 * elements.  Unknown keys (e.g. the duplicate `new_conv.*`, unet.py:182,233) are
 * ignored; a missing or mis-sized required key fails with LDMSEG_E_WEIGHT.
 * Replaces: UNet.from_pretrained + remove_cross_attention + modify_encoder +
 * load_state_dict (tools/main_ldm.py:146-168, trainers_ldm_cond.py:1863-1891).
 *
 * Separate image encoder (modify_encoder(separate_encoder=True[, add_adaptor=True]), unet.py:42-63): a state dict that holds
 * `conv_in_img.weight` makes a separate-encoder handle.  It must then hold conv_in.* and conv_in_img.* with 4 input channels,
 * `down_blocks_additional.*` (key for key the down_blocks of a UNet without cross-attention) and may hold
 * `adaptor_layers.{0..3}.{weight,bias}` (3x3, C -> C per level).  cfg.in_channels must be 8 and cfg.cross_attention 0, else
 * LDMSEG_E_ARG.  Such a handle takes the 8-channel input [segmentation | RGB latents]; conv_in sees the first half, the image
 * branch the second together with emb(timestep_img), and its 12 outputs are added to the 12 skip connections (unet.py:309-385).
 * A `separate_conv` checkpoint (conv_in_seg.*) is an ordinary 8-channel conv_in once folded: ldmseg_amd.checkpoint does that. */
int ldmseg_unet_create(const ldmseg_unet_cfg* cfg, int n_weights, const char* const* names,
                       const void* const* dev_ptrs, const int64_t* numels, ldmseg_unet** out);
void ldmseg_unet_destroy(ldmseg_unet* h);

/* UNet.forward(sample, timestep, encoder_hidden_states=None).sample  (unet.py:281-436).
 * x: [B, in_channels, L, L] fp32; out: [B, 4, L, L] fp32.  The timestep is read from
 * `t_dev` (int64 on device, `t_count` = 1 -> broadcast like timestep.expand(B), or B)
 * so a GPU-resident scheduler.timesteps[i] needs no D2H sync; if t_dev is NULL,
 * `t_host` is used.  L must be a multiple of 8. */
int ldmseg_unet_forward(ldmseg_unet* h, const float* x, const int64_t* t_dev, int t_count, int64_t t_host,
                        int B, int L, float* out, void* stream);
/* Same forward but the input is given as its channel-concat parts
 * (torch.cat([latents, rgb_latents, condition], dim=1), trainers_ldm_cond.py:1128-1138);
 * `cond` may be NULL when in_channels == 8. */
int ldmseg_unet_forward_parts(ldmseg_unet* h, const float* latents, const float* rgb_latents, const float* cond,
                              const int64_t* t_dev, int t_count, int64_t t_host, int B, int L, float* out,
                              void* stream);
/* UNet.forward(sample, timestep, None, timestep_img=...).sample (unet.py:281-436): ldmseg_unet_forward with the timestep of the
 * separate image encoder, given like the timestep itself (timg_dev int64 on the device with timg_count = 1 or B entries, or, NULL,
 * timg_host); timg_count other than 1 or B is LDMSEG_E_ARG.  ldmseg_unet_forward and ldmseg_unet_forward_parts on a
 * separate-encoder handle mean timestep_img = 0 (what the reference substitutes for None); all three compute the image branch
 * inside the call.  On any other handle timestep_img is ignored, as the reference ignores it there. */
int ldmseg_unet_forward_img(ldmseg_unet* h, const float* x, const int64_t* t_dev, int t_count, int64_t t_host,
                            const int64_t* timg_dev, int timg_count, int64_t timg_host, int B, int L, float* out, void* stream);
/* UNet.forward(sample, timestep, encoder_hidden_states=ctx).sample of a cross-attention handle (unet.py:281-436 with
 * attn2 kept).  ctx: [B, S, ctx_dim] fp32 on the device, 1 <= S <= 4096 (77 CLIP text tokens, 257 CLIP-L/14 patch features,
 * 1 projected image embedding - the last two are what ldmseg_clip_vision_describe / _forward below produce); ctx_dim = 768,
 * or 1024 when the handle holds encoder_hid_proj (applied once per call, unet.py:319-320).  The context's keys / values for all 16 transformers are computed once per call into the workspace
 * (planned for the last S / ctx_dim used: a call with another context shape re-plans and may synchronise).  LDMSEG_E_ARG on a
 * handle without cross-attention; the plain ldmseg_unet_forward / _forward_parts return LDMSEG_E_ARG on a cross handle. */
int ldmseg_unet_forward_ctx(ldmseg_unet* h, const float* x, const int64_t* t_dev, int t_count, int64_t t_host, int B, int L,
                            const float* ctx, int S, int ctx_dim, float* out, void* stream);
/* bf16 mode only: run the self-attention of every level with at least `min_tokens` tokens (H*W) on the fp8 operand path
 * (OCP e4m3 Q/K/V/P on v_mfma_f32_16x16x32_fp8_fp8, fp32 accumulation and statistics) - the "fp8 MFMA attention path" of
 * the 1024x1024 configuration (128x128 latents: 16384 / 4096 tokens at head dims 40 / 80); 0 switches it off (default).
 * Levels where the fp8 path is not the faster one (head dim 80 / token counts that are not a multiple of 128: only the unscaled
 * fp8 MFMAs serve them, at the bf16 rate) stay on the bf16 kernel whatever `min_tokens` says.
 * The reference has no counterpart (its attention is whatever diffusers' processor does in fp32). */
int ldmseg_unet_set_attention_fp8(ldmseg_unet* h, int min_tokens);
/* Allocate everything forward / sample_loop need at (B, L) now (workspace + the sampler's eps,
 * self-condition and time-embedding buffers); may synchronise the device.  Optional: without it the first call at a new,
 * larger shape does the same lazily. */
int ldmseg_unet_reserve(ldmseg_unet* h, int B, int L);
/* Workgroups of this handle's cooperative GroupNorm launches that did not see their partners within the poll bound and
 * computed the partners' statistics themselves since the handle was created, launches under the back-off's short bound
 * excepted (0 on an undisturbed device: the kernel's workgroups are co-resident).  Synchronises.  ldmseg_sample_loop looks at the same counter (asynchronously) and runs the
 * next calls with a short poll bound while it grows.  No reference counterpart (torch's GroupNorm is one kernel). */
int ldmseg_unet_gn_fallbacks(ldmseg_unet* h, int64_t* count);
/* Workgroups of this handle's K-sliced GEMM launches that gave up waiting for the other slices of their tile (poll bound 200 us) and
 * left their share of the reduction to the tile's last arriver, since the handle was created (0 on an undisturbed device).  Results
 * are the same either way; the counter says whether something else is holding CUs.  Synchronises.  No reference counterpart. */
int ldmseg_unet_cf_fallbacks(ldmseg_unet* h, int64_t* count);
/* ldmseg_sample_loop calls this handle will still run with the short (2 us) partner poll: 8 after a call whose full-bound norms
 * missed their partners at least 256 times, one less after every call; launches under the short bound do not count, so the
 * call after the eighth tries the full bound again.  Does not synchronise (the loop reads the counter one call late). */
int ldmseg_unet_gn_backoff(ldmseg_unet* h, int32_t* calls_left);
/* bytes of device workspace a forward at (B, L) needs (allocated lazily, grown never shrunk) */
size_t ldmseg_unet_workspace_bytes(const ldmseg_unet* h, int B, int L);
/* number of parameters held (815,556,484 for the 12-channel default; 859,532,484 for an 8-channel cross-attention handle,
 * 860,319,684 with encoder_hid_proj; 1,049,661,444 for a separate-encoder handle, 1,083,764,164 with adaptor layers) */
int64_t ldmseg_unet_num_params(const ldmseg_unet* h);

/* ---- seg-VAE: ldmseg/models/vae.py::GeneralVAESeg (gaussian, num_mid_blocks=0) ------------ */
typedef struct {
  int32_t in_channels;      /* 7  (bit maps, base.yaml:15) */
  int32_t int_channels;     /* 256 */
  int32_t out_channels;     /* 128 */
  int32_t latent_channels;  /* 4 */
  int32_t num_latents;      /* 2 (mean, logvar) */
  int32_t num_upscalers;    /* 2 */
  int32_t upscale_channels; /* 256 */
  int32_t norm_num_groups;  /* 32 */
  int32_t block_out_channels[4]; /* 32,64,128,256 */
  int32_t compute_dtype;
  int32_t device;
} ldmseg_vae_cfg;

/* keys: encoder.{0,2,3,5,6,8,9,11,13,15}.{weight,bias}, decoder.{0,2,3,5,6,8,10}.{weight,bias}
 * (vae.py:123-244; the AE checkpoint's 'module.' prefix is stripped by the caller, vae.py:116-121) */
int ldmseg_vae_create(const ldmseg_vae_cfg* cfg, int n_weights, const char* const* names,
                      const void* const* dev_ptrs, const int64_t* numels, ldmseg_vae** out);
void ldmseg_vae_destroy(ldmseg_vae* h);
/* GeneralVAESeg.decode(z, interpolate) (vae.py:267-271): z [B,4,L,L] -> logits
 * [B,128,4L,4L] (interpolate=0) or [B,128,8L,8L] (bilinear x2, align_corners=False).
 * `z_scale` multiplies z first (decode_latents' 1/scaling_factor, trainers_ldm_cond.py:421). */
int ldmseg_vae_decode(ldmseg_vae* h, const float* z, float z_scale, int B, int L, int interpolate, float* logits,
                      void* stream);
/* Backward of decode(z, interpolate=False): from grad_logits [B,Co,4L,4L] (fp32 NCHW, d loss / d logits) to the gradient
 * of every decoder parameter asked for and of the latents.  Stateless: the decoder forward runs again inside the call's own workspace
 * plan (one extra decoder forward), so nothing is carried from an earlier decode and other calls on the handle in between are
 * harmless.  Everything on `stream`, no allocation after the plan, no host synchronisation, bitwise repeatable (no float atomics).
 * grad_z [B,4,L,L] or NULL; it includes the z_scale factor.  names[i] is a reference key (decoder.0.weight ...), grad_ptrs[i] an
 * fp32 device buffer of numels[i] elements in the state-dict layout ([Co,Ci,3,3], [Ci,Co,2,2], [C]), every element written.  A key
 * that is absent, or a NULL pointer, skips that gradient; an unknown key or a wrong numel is LDMSEG_E_ARG, as is a bf16 handle (the
 * backward needs an fp32-storage handle: compute_dtype fp32 or bf16x3).  Nothing is launched on an error. */
int ldmseg_vae_decode_backward(ldmseg_vae* h, const float* z, float z_scale, int B, int L, const float* grad_logits, float* grad_z,
                               int n, const char* const* names, float* const* grad_ptrs, const int64_t* numels, void* stream);
/* Repacks the given decoder tensors (reference keys, fp32 device pointers) into the buffers the handle already owns: forward
 * packing, data-gradient packing, the hi | lo planes of a bf16x3 handle, norm and bias vectors.  Afterwards every entry of the
 * handle computes with the new values, bitwise as a handle created from them.  Nothing is allocated; the launches are on
 * `stream`.  An unknown key or a wrong numel is LDMSEG_E_ARG. */
int ldmseg_vae_load_decoder(ldmseg_vae* h, int n, const char* const* names, const void* const* dev_ptrs, const int64_t* numels,
                            void* stream);
/* Fused tail of TrainerDiffusion.decode_latents(return_logits=False, threshold_output) (trainers_ldm_cond.py:
 * 421-433): decode -> bilinear x2 -> argmax over the 128 classes and max-softmax probability, without writing the
 * logits.  ids [B,8L,8L] int64 (= ignore_label where max prob < mask_th; mask_th < 0 disables the threshold),
 * max_prob [B,8L,8L] fp32 or NULL. */
int ldmseg_vae_decode_argmax(ldmseg_vae* h, const float* z, float z_scale, int B, int L, float mask_th, int64_t ignore_label,
                             int64_t* ids, float* max_prob, void* stream);
/* The evaluation tail of TrainerDiffusion.compute_pq (trainers_ldm_cond.py:1243-1313) in one call, without the
 * [B,128,H,W] fp32 logits: decode (vae.py:267-271 incl. the bilinear x2) -> F.interpolate to the network input size
 * (in_h, in_w) (:1252-1257) -> crop_padding (:1172-1178, :1263) -> F.interpolate to the original size (h_b, w_b)
 * (:1266-1271) -> argmax / thresholds / segment filtering (:1277-1313, see ldmseg_panoptic_postprocess below).  The
 * three bilinear stages (all align_corners=False) are evaluated as one separable weighted sum over the decoder's 4L map.
 *   crop_boxes  [B][4] HOST int32 (y0, x0, height, width) of the non-padded box in the (in_h, in_w) grid; NULL = whole grid
 *   out_sizes   [B][2] HOST int32 (h_b, w_b);  out_offsets [B] HOST int64: first element of image b in labels / panoptic
 *   labels, panoptic: flat int32 device buffers holding the ragged [h_b * w_b] maps; keep / counts / mask_counts [B,C]
 * as in ldmseg_panoptic_postprocess.  Enqueues 2B + 2 small launches behind the decoder. */
int ldmseg_vae_decode_panoptic(ldmseg_vae* h, const float* z, float z_scale, int B, int L, int in_h, int in_w,
                               const int32_t* crop_boxes, const int32_t* out_sizes, const int64_t* out_offsets,
                               int threshold_output, int threshold_mode, float mask_th, int count_th, double overlap_th,
                               int64_t ignore_label, int32_t* labels, int32_t* panoptic, uint8_t* keep, int32_t* counts,
                               int32_t* mask_counts, void* stream);
/* Panoptic post-processing of the evaluation loop (trainers_ldm_cond.py:1277-1313) on logits [B,C,H,W] fp32 that
 * are already at the output size (C <= 256):
 *   labels   [B,H,W] int32  argmax over C; -1 where threshold_output and (threshold_mode 0: max softmax prob,
 *                           1 'topk_diff': top1 - top2 prob) < mask_th                       (:1277-1286)
 *   counts   [B,C]  int32   pixels per label (np.unique counts, :1295)
 *   mask_counts [B,C] int32 pixels with sigmoid(logit_c) >= mask_th (original_mask.sum(), :1303)
 *   keep     [B,C]  uint8   0 where label == ignore_label, counts < count_th or counts / mask_counts < overlap_th
 *                           (:1298-1306); kept labels are the reference's segments_info ids (c + 1)
 *   panoptic [B,H,W] int32  label + 1 where kept, 0 (void) elsewhere                          (:1300,1305,1313)
 * All outputs are device buffers owned by the caller.  One pass over the logits; nothing is copied to the host. */
int ldmseg_panoptic_postprocess(const float* logits, int B, int C, int H, int W, int threshold_output, int threshold_mode,
                                float mask_th, int count_th, double overlap_th, int64_t ignore_label, int32_t* labels,
                                int32_t* panoptic, uint8_t* keep, int32_t* counts, int32_t* mask_counts, void* stream);
/* GeneralVAESeg.encode(x) (vae.py:252-265): x [B,7,H,W] (H=W multiple of 8), moments
 * [B,8,H/8,W/8] = (mean | logvar) before the clamp.  x is used as x*in_mul+in_add
 * (encode_inputs' 2x-1, trainers_ldm_cond.py:369). */
int ldmseg_vae_encode(ldmseg_vae* h, const float* x, float in_mul, float in_add, int B, int H, float* moments,
                      void* stream);
/* DiagonalGaussianDistribution.mode()/.sample() (vae.py:370-413) on `moments`:
 * out[B,4,l,l] = (mean + exp(0.5*clamp(logvar,-30,20))*noise) * out_scale; noise NULL -> mode(). */
int ldmseg_vae_posterior(const float* moments, const float* noise, float out_scale, int B, int l, float* out,
                         void* stream);
/* Backward of ldmseg_vae_posterior to the moments: grad_moments [B,8,l,l] = (d mean | d logvar) from grad_z [B,4,l,l] (the gradient
 * of `out`, so `scale` = the out_scale of the forward): d mean = scale * grad_z, d logvar = scale * grad_z * noise * 0.5 * std where
 * -30 <= logvar <= 20 (bounds included, as torch.clamp passes gradient) and 0 elsewhere; noise NULL (mode()): the logvar half is
 * exact zeros.  Every element of grad_moments is written. */
int ldmseg_vae_posterior_backward(const float* moments, const float* noise, float scale, int B, int l, const float* grad_z,
                                  float* grad_moments, void* stream);
/* Backward of ldmseg_vae_encode: from grad_moments [B,8,H/8,H/8] (fp32 NCHW) to the gradient of every encoder
 * parameter asked for.  Stateless, like ldmseg_vae_decode_backward: the encoder forward runs again inside the call's own workspace
 * plan, keeping what the backward reads (the four conv + SiLU layers keep their pre-activation).  Everything on `stream`, no
 * allocation after the plan, no host synchronisation, bitwise repeatable (no float atomics).  names / grad_ptrs / numels as in
 * ldmseg_vae_decode_backward with the encoder's reference keys (encoder.0.weight [32,7,3,3] ... encoder.15.bias): real channels
 * only, every element written; an absent key or a NULL pointer skips that gradient and leaves the others bitwise unchanged; an
 * unknown key, a wrong numel or a bf16 handle is LDMSEG_E_ARG and nothing is launched.  The input is data: it gets no gradient. */
int ldmseg_vae_encode_backward(ldmseg_vae* h, const float* x, float in_mul, float in_add, int B, int H, const float* grad_moments,
                               int n, const char* const* names, float* const* grad_ptrs, const int64_t* numels, void* stream);
/* ldmseg_vae_load_decoder for the encoder's tensors (encoder.0.weight ...): forward packing, the data-gradient packings of an
 * fp32-storage handle, the hi | lo planes of a bf16x3 handle, norm and bias vectors.  Nothing is allocated. */
int ldmseg_vae_load_encoder(ldmseg_vae* h, int n, const char* const* names, const void* const* dev_ptrs, const int64_t* numels,
                            void* stream);
/* ---- stage-1 (seg-VAE reconstruction) evaluation: TrainerAE.compute_metrics(['miou', 'pq']), trainers_ae.py:546-803 ---- */
/* SemsegMeter.update(pred, gt) (ldmseg/evaluations/semseg_evaluation.py:24-33) on n int64 (pred, gt) pairs on the device.
 * counts int64 [3][num_classes] = (tp | fp | fn) is ADDED to, never reset: per pixel with gt != ignore_index,
 *   pred == gt, 0 <= gt < K: tp[gt] += 1;  pred != gt, 0 <= gt < K: fn[gt] += 1;  pred != gt, 0 <= pred < K: fp[pred] += 1
 * (the three masked sums of :31-33 read per pixel).  num_classes <= 256.  One launch, no host synchronisation. */
int ldmseg_semseg_meter_update(const int64_t* pred, const int64_t* gt, int64_t n, int num_classes, int64_t ignore_index,
                               int64_t* counts, void* stream);
/* The tail of TrainerAE.compute_miou (trainers_ae.py:754-761) fused behind the decoder, without the [B,128,out_h,out_w]
 * fp32 logits: decode(z * z_scale, interpolate=False) (vae.py:267-271) -> F.interpolate(size=(out_h, out_w), bilinear,
 * align_corners=True) (:754) -> argmax (:755) -> pred = ignore_label where max softmax prob < mask_th (:757-760; mask_th < 0
 * disables it) -> SemsegMeter.update(pred, targets) (:761) into counts as in ldmseg_semseg_meter_update.
 *   targets [B,out_h,out_w] int64 device or NULL;  preds [B,out_h,out_w] int64 device or NULL;  counts [3][num_classes] or NULL
 * (targets and counts are used together: with either NULL no counter is touched). */
int ldmseg_vae_decode_semseg(ldmseg_vae* h, const float* z, float z_scale, int B, int L, int out_h, int out_w, float mask_th,
                             int64_t ignore_label, const int64_t* targets, int64_t ignore_index, int num_classes, int64_t* preds,
                             int64_t* counts, void* stream);
/* vae_model(images, sample_posterior=False).sample (vae.py:273-307; trainers_ae.py:752) plus that tail in one call:
 * encode(x * in_mul + in_add) -> posterior mode -> decode(interpolate=False), no scaling factor; x [B,7,H,H], H a multiple of 8.
 * Moments and latents stay in the handle's workspace, whose plan covers encoder and decoder together. */
int ldmseg_vae_reconstruct_semseg(ldmseg_vae* h, const float* x, float in_mul, float in_add, int B, int H, int out_h, int out_w,
                                  float mask_th, int64_t ignore_label, const int64_t* targets, int64_t ignore_index,
                                  int num_classes, int64_t* preds, int64_t* counts, void* stream);
/* TrainerAE.compute_pq's per-batch work (trainers_ae.py:611-668) in one call: the same reconstruction chain into the tail of
 * ldmseg_vae_decode_panoptic (resize to (in_h, in_w) :614-619, crop :626, resize to the original size :629-634, argmax /
 * max-softmax threshold :637-641, segment filter :648-659) with ONE difference: the overlap mask is logit >= mask_th on the raw
 * logits (:656), not sigmoid(logit) >= mask_th.  Geometry arrays and outputs as in ldmseg_vae_decode_panoptic. */
int ldmseg_vae_reconstruct_panoptic(ldmseg_vae* h, const float* x, float in_mul, float in_add, int B, int H, int in_h, int in_w,
                                    const int32_t* crop_boxes, const int32_t* out_sizes, const int64_t* out_offsets,
                                    int threshold_output, float mask_th, int count_th, double overlap_th, int64_t ignore_label,
                                    int32_t* labels, int32_t* panoptic, uint8_t* keep, int32_t* counts, int32_t* mask_counts,
                                    void* stream);
/* ---- device-side panoptic-quality meter: pq_compute_annotations (the restated panopticapi rule) for a batch of map pairs ----
 * Per image b: the prediction map (int32, label + 1, 0 = void, ids 0..P, P <= 256) at pred + pred_offsets[b] and the ground-truth
 * map of the same (h_b, w_b) = sizes[b] at pixel gt_offsets[b] of gt, in gt_format 0 (int32 segment ids) or 1 (uint8 RGB
 * [h,w,3], id = R + 256 G + 65536 B).  keep [B][P] uint8 declares prediction id p where keep[b][p - 1] != 0 (the keep table of
 * ldmseg_vae_decode_panoptic with C = P).  The annotation's declared segments are slots 0..gt_counts[b]-1 in ASCENDING id order:
 *   slot_ids   [B][Gpad] int32   ids, 1 .. 2^24 - 1          slot_crowd [B][Gpad] uint8  iscrowd
 *   slot_area  [B][Gpad] int64   area, or -1 = the counted one (gt_segms[g].setdefault("area", count))
 *   slot_meta  [B][2]    int32   (gt_counts[b], slot of the LAST crowd segment in annotation order or -1)
 * with gt_counts[b] <= Gpad <= LDMSEG_PQ_G_MAX.  sizes [B][2], pred_offsets [B], gt_offsets [B], gt_counts [B] are HOST arrays,
 * everything else lives on the device.  Outputs (device, owned by the caller, (re)initialised by the call):
 *   inter     [B][Gpad + 2][P + 1] int32  pixel counts; row 0 = VOID, rows 1..G = slots, row G + 1 = painted but not declared
 *   stats     [B][4] int32  tp, fp, fn, flags: bit 0 a painted prediction id >= 1 is not declared, bit 1 a declared prediction
 *             id has no pixel, bit 2 a prediction id outside 0..P, bit 3 a segment matched twice or an empty union (only
 *             annotation areas that contradict the map do that; the slot table cannot hold such a result)
 *   match_iou [B][Gpad] double  the matched IoU (> 0.5) of the slot, 0.0 elsewhere
 * A pair (slot g not crowd, declared p) with n = inter[g][p] > 0 matches iff (double)n / (double)(area_pred[p] + area_gt[g] - n -
 * inter[VOID][p]) > 0.5; fn = unmatched non-crowd slots; fp = unmatched declared p unless (inter[VOID][p] + inter[last crowd][p]) /
 * area_pred[p] > 0.5.  Integer atomics and IEEE double divisions only: the result is exact and order-independent.
 * B + 1 launches, no host synchronisation, no allocation. */
#define LDMSEG_PQ_G_MAX 256
int ldmseg_pq_match(const int32_t* pred, const void* gt, int gt_format, int B, const int32_t* sizes, const int64_t* pred_offsets,
                    const int64_t* gt_offsets, const uint8_t* keep, int P, const int32_t* gt_counts, int Gpad,
                    const int32_t* slot_ids, const uint8_t* slot_crowd, const int64_t* slot_area, const int32_t* slot_meta,
                    int32_t* inter, int32_t* stats, double* match_iou, void* stream);
int64_t ldmseg_vae_num_params(const ldmseg_vae* h);

/* ---- image VAE encoder: ldmseg/models/vae.py:36-39 GeneralVAEImage(AutoencoderKL), decoder removed
 * (tools/main_ldm.py:137-139); used as encode_func in TrainerDiffusion.encode_inputs (trainers_ldm_cond.py:360-375).
 * SD-1.x VAE encoder: conv_in 3->128, down blocks 128/256/512/512 with two temb-free resnets each (GroupNorm 32,
 * eps 1e-6, SiLU), stride-2 convs with F.pad(0,1,0,1), mid block resnet / single-head attention (C=512) / resnet,
 * conv_norm_out + SiLU + conv_out 512->8, quant_conv 8->8.  The arithmetic is diffusers' (not vendored by the
 * reference): parity is pinned against oracle/vae_image.py only. */
typedef struct {
  int32_t compute_dtype;    /* LDMSEG_F32 | LDMSEG_BF16 | LDMSEG_BF16X3 */
  int32_t device;
} ldmseg_vae_image_cfg;
/* keys: the 'vae_image' entry of ldmseg.pt (trainers_ldm_cond.py:1805) / AutoencoderKL.state_dict():
 * encoder.conv_in, encoder.down_blocks.{0..3}.resnets.{0,1}.{norm1,conv1,norm2,conv2[,conv_shortcut]},
 * encoder.down_blocks.{0..2}.downsamplers.0.conv, encoder.mid_block.resnets.{0,1}.*,
 * encoder.mid_block.attentions.0.{group_norm, query|to_q, key|to_k, value|to_v, proj_attn|to_out.0},
 * encoder.conv_norm_out, encoder.conv_out, quant_conv (decoder.* / post_quant_conv.* are ignored). */
int ldmseg_vae_image_create(const ldmseg_vae_image_cfg* cfg, int n_weights, const char* const* names,
                            const void* const* dev_ptrs, const int64_t* numels, ldmseg_vae_image** out);
void ldmseg_vae_image_destroy(ldmseg_vae_image* h);
int64_t ldmseg_vae_image_num_params(const ldmseg_vae_image* h);
/* AutoencoderKL.encode(x).latent_dist parameters: x [B,3,H,W] fp32 (used as x*in_mul+in_add: encode_inputs' 2x-1,
 * trainers_ldm_cond.py:369), H, W multiples of 8 with (H/8)*(W/8) a multiple of 64 -> moments [B,8,H/8,W/8]
 * (mean | logvar before the clamp); feed ldmseg_vae_posterior for .mode()/.sample() and the scaling factor. */
int ldmseg_vae_image_encode(ldmseg_vae_image* h, const float* x, float in_mul, float in_add, int B, int H, int W,
                            float* moments, void* stream);

/* ------------------------------------------------------------------ CLIP image encoder (image descriptors)
 * The image descriptor of image_descriptors = clip_image / clip_image_proj: transformers' CLIPVisionModel /
 * CLIPVisionModelWithProjection behind MyCLIPVisionModel / MyCLIPVisionModelWithProjection (ldmseg/models/descriptors.py:15-56,
 * 67-76, called at trainers_ldm_cond.py:1102-1103).  Patch conv (stride = patch, no bias) + class token + position table,
 * pre_layrnorm, num_layers pre-norm blocks (self-attention with head dim 64, quick-GELU MLP), last_hidden_state WITHOUT the
 * post-layernorm, pooled = post_layernorm(class row), image_embeds = visual_projection(pooled).  All LayerNorms eps 1e-5.
 * The arithmetic is transformers' (not vendored by the reference): parity is pinned against tests/clip_vision_ref.py, which
 * the CPU suite pins against transformers itself. */
typedef struct ldmseg_clip_vision ldmseg_clip_vision;  /* opaque */
typedef struct {
  int32_t hidden_size;        /* 1024; 64 * num_heads, at most 1280 (the widest row the LayerNorm statistics kernel serves in fp32) */
  int32_t intermediate_size;  /* 4096; a multiple of 64 */
  int32_t num_layers;         /* 24 */
  int32_t num_heads;          /* 16; hidden_size / num_heads must be 64 */
  int32_t image_size;         /* 224; a multiple of patch_size */
  int32_t patch_size;         /* 14 */
  int32_t projection_dim;     /* 768, or 0: no visual_projection (clip_image) */
  int32_t compute_dtype;      /* LDMSEG_F32 | LDMSEG_BF16 | LDMSEG_BF16X3 */
  int32_t device;
} ldmseg_clip_vision_cfg;
/* keys: CLIPVisionModel.state_dict() without the `vision_model.` prefix - embeddings.{class_embedding, patch_embedding.weight,
 * position_embedding.weight}, pre_layrnorm.{weight,bias} (sic), encoder.layers.{i}.{layer_norm1, self_attn.{q,k,v,out}_proj,
 * layer_norm2, mlp.fc1, mlp.fc2}.{weight,bias}, post_layernorm.{weight,bias} - plus visual_projection.weight when
 * projection_dim > 0 (embeddings.position_ids is ignored).  LDMSEG_E_SHAPE for a configuration the kernels do not serve. */
int ldmseg_clip_vision_create(const ldmseg_clip_vision_cfg* cfg, int n_weights, const char* const* names,
                              const void* const* dev_ptrs, const int64_t* numels, ldmseg_clip_vision** out);
void ldmseg_clip_vision_destroy(ldmseg_clip_vision* h);
int64_t ldmseg_clip_vision_num_params(const ldmseg_clip_vision* h);
/* CLIPVisionModel(pixel_values).last_hidden_state -> last_hidden [B, T, hidden] (T = (image/patch)^2 + 1) and
 * CLIPVisionModelWithProjection(pixel_values).image_embeds -> image_embeds [B, projection_dim]; pixel_values [B,3,S,S] fp32,
 * already resized and normalised.  Either output may be NULL; image_embeds on a handle without projection: LDMSEG_E_ARG. */
int ldmseg_clip_vision_forward(ldmseg_clip_vision* h, const float* pixel_values, int B, float* last_hidden, float* image_embeds,
                               void* stream);
/* The same from raw images rgb [B,3,H,W] in [0,1], any H, W >= 1: norm_resize_images (trainers_ldm_cond.py:663-675) -
 * F.interpolate(rgb, (S,S), mode='bilinear', align_corners=False) without antialias, then (x - mean) / std per channel - runs
 * inside the kernel that writes the patch rows. */
int ldmseg_clip_vision_describe(ldmseg_clip_vision* h, const float* rgb, int B, int H, int W, const float mean[3],
                                const float std[3], float* last_hidden, float* image_embeds, void* stream);

/* ---- CLIP text encoder: the conditioning model of image_descriptors `none` ------------------ */
/* transformers CLIPTextModel, SD-1.x's text_encoder (loaded at ldmseg/models/descriptors.py:98-103, called on the tokenised
 * prompts and on the empty prompts at trainers_ldm_cond.py:1108-1119, which read [0] = last_hidden_state).  Token + position
 * embedding, num_layers pre-norm blocks (CAUSAL self-attention with head dim 64, quick-GELU MLP), final_layer_norm on every
 * row.  All LayerNorms eps 1e-5; no padding mask (the reference passes none).  pooler_output is not computed: nothing reads
 * it.  The arithmetic is transformers' (not vendored by the reference): parity is pinned against tests/clip_text_ref.py,
 * which the CPU suite pins against transformers itself. */
typedef struct ldmseg_clip_text ldmseg_clip_text;  /* opaque */
typedef struct {
  int32_t vocab_size;         /* 49408 */
  int32_t max_positions;      /* 77 */
  int32_t hidden_size;        /* 768; 64 * num_heads, at most 1280 */
  int32_t intermediate_size;  /* 3072; a multiple of 64 */
  int32_t num_layers;         /* 12 */
  int32_t num_heads;          /* 12 */
  int32_t compute_dtype;      /* LDMSEG_F32 | LDMSEG_BF16 | LDMSEG_BF16X3 */
  int32_t device;
} ldmseg_clip_text_cfg;
/* keys: CLIPTextModel.state_dict() without the `text_model.` prefix - embeddings.{token_embedding,position_embedding}.weight,
 * encoder.layers.{i}.{layer_norm1, self_attn.{q,k,v,out}_proj, layer_norm2, mlp.fc1, mlp.fc2}.{weight,bias},
 * final_layer_norm.{weight,bias} (embeddings.position_ids is ignored).  Both embedding tables stay fp32 in the handle.
 * LDMSEG_E_SHAPE for a configuration the kernels do not serve (the limits of the vision handle). */
int ldmseg_clip_text_create(const ldmseg_clip_text_cfg* cfg, int n_weights, const char* const* names,
                            const void* const* dev_ptrs, const int64_t* numels, ldmseg_clip_text** out);
void ldmseg_clip_text_destroy(ldmseg_clip_text* h);
int64_t ldmseg_clip_text_num_params(const ldmseg_clip_text* h);
/* CLIPTextModel(input_ids).last_hidden_state -> last_hidden [R, T, hidden] fp32; input_ids_dev: int64 [R, T] on the device,
 * 1 <= T <= max_positions (LDMSEG_E_SHAPE otherwise).  Ids are clamped to [0, vocab_size) for memory safety only: checking
 * their range is the caller's job (the Python wrapper raises IndexError).  The workspace is planned per (R, T), grows
 * lazily and never shrinks. */
int ldmseg_clip_text_forward(ldmseg_clip_text* h, const int64_t* input_ids_dev, int R, int T, float* last_hidden, void* stream);

/* ---- scheduler: ldmseg/schedulers/ddim_scheduler.py --------------------------------------- */
/* DDIMNoiseScheduler.step (:218-269), elementwise over n floats.  The four coefficients are
 * the 0-d fp32 values the reference computes on the host (alpha_prod_t**0.5, ...); every
 * product/sum is rounded separately, so outputs equal the torch result bit for bit.
 * prev or x0 may be NULL. */
int ldmseg_ddim_step(const float* model_output, const float* sample, float sqrt_alpha_t, float sqrt_beta_t,
                     float sqrt_alpha_prev, float sqrt_beta_prev, int prediction_type, int clip_sample,
                     float clip_sample_range, int use_clipped_model_output, float* prev_sample,
                     float* pred_original_sample, size_t n, void* stream);
/* add_noise (:155-187) / remove_noise (:190-216) with per-sample int64 timesteps [B] and the
 * fp32 alphas_cumprod table [n_train_timesteps] on device.  The reference raises IndexError for a
 * timestep outside [0, n_train_timesteps); device-resident timesteps cannot be inspected without a
 * sync, so the kernel clamps the index into the table (never an out-of-bounds read) and the Python
 * wrapper raises IndexError whenever it is handed host-resident timesteps. */
int ldmseg_add_noise(const float* original, const float* noise, const int64_t* timesteps_dev,
                     const float* alphas_cumprod_dev, int n_train_timesteps, float scale, float* out, int B,
                     size_t per_sample, void* stream);
int ldmseg_remove_noise(const float* noisy, const float* noise, const int64_t* timesteps_dev,
                        const float* alphas_cumprod_dev, int n_train_timesteps, float scale, float* out, int B,
                        size_t per_sample, void* stream);

/* ---- denoising loss: the forward half of the training step (trainers_ldm_cond.py:445-661) -------------------- */
#define LDMSEG_LOSS_L1 0
#define LDMSEG_LOSS_L2 1
#define LDMSEG_LOSS_SMOOTH_L1 2          /* beta = 1 */
/* Everything of compute_loss / predict_sample behind the UNet forward (:594-615, :483-492), on [B,C,HW] fp32 tensors:
 *   element loss  l1 |x - y|, l2 (x - y) * (x - y), smooth_l1 (z < 1 ? 0.5 * z * z : z - 0.5), x = prediction, y = target
 *                 (:515-520), times loss_mask[b][pixel] (:525) if given, times weights_dev[t_b] (:597) if given; every product
 *                 and difference rounded separately, bit-identical to the reference's fp32 values.  Written to elem_loss if
 *                 non-NULL.  target NULL: no loss at all (mean / sample_sums / elem_loss are not written).
 *   pred_latents  (if non-NULL) prediction_type 0 'epsilon': remove_noise(noisy, prediction, t) with ldmseg_remove_noise's own
 *                 arithmetic (scale 1); 1 'sample': prediction (:605-611); then paste_src where paste_mask != 0 (:614-615);
 *                 then clamp(., minmax_dev[0], minmax_dev[1]) (:492) if minmax_dev is non-NULL (ldmseg_tensor_minmax's pair; a NaN bound
 *                 makes every value NaN, like torch.clamp).
 *   sample_sums   [B] fp32 (may be NULL): the sample's element losses added in fp64, rounded once.
 *   mean          [1] fp32: ohem_ratio >= 1: sum of all element losses (fp64) / (B*C*HW).  ohem_ratio < 1 (needs elem_loss):
 *                 torch.topk(loss.view(-1), k)[0].mean() with k = (int64)(ohem_ratio * (double)(B*C*HW)) (:600-602), exact: a
 *                 radix select over the bit patterns finds the k-th largest value, the strictly larger elements are added in
 *                 fp64 and the ties enter as count * value.  k == 0 is LDMSEG_E_ARG.  A NaN element makes the mean NaN.
 * Workgroups store fp64 partial sums that one finishing launch adds in a fixed order: no float atomics, two calls on the same
 * inputs agree bit for bit.  timesteps_dev [B] int64 is clamped into the table like ldmseg_add_noise.  paste_mask is uint8 / bool
 * [B,C,HW].  scratch: ldmseg_diffusion_loss_scratch_bytes(B, C, HW) bytes of device memory, owned by the caller, reusable by a
 * later call on the same stream.  2 launches (7 + one memset node with OHEM); no host synchronisation, no allocation. */
size_t ldmseg_diffusion_loss_scratch_bytes(int B, int C, int HW);
int ldmseg_diffusion_loss(const float* prediction, const float* target, const float* noisy, const int64_t* timesteps_dev,
                          const float* alphas_cumprod_dev, int n_train_timesteps, const float* weights_dev,
                          const float* loss_mask, const uint8_t* paste_mask, const float* paste_src, const float* minmax_dev,
                          int loss_type, int prediction_type, double ohem_ratio, int B, int C, int HW, float* elem_loss,
                          float* pred_latents, float* mean, float* sample_sums, void* scratch, void* stream);
/* get_loss_weight_mask (:643-661): src [B,Hi,Wi] (src_dtype 0 int64, 1 uint8 / bool, 2 fp32) -> out [B,h,w] fp32 through the source
 * pixel of F.interpolate(mode='nearest').  LDMSEG_MASK_IGNORE: value != ignore_label; LDMSEG_MASK_PADDING: the resized value;
 * LDMSEG_MASK_COUNTS: 1 / (pixels of the same id in the resized map of the image), 0 on ignore_label.  COUNTS keeps one 256-entry
 * table per image: an id outside [0, 256) (the bit codec's range) sets bit 0 of *flag (device int32, reset by the call) and gets
 * the weight NaN, so that it can neither index out of bounds nor go unnoticed in the loss.  One launch, one workgroup per image. */
#define LDMSEG_MASK_IGNORE 0
#define LDMSEG_MASK_PADDING 1
#define LDMSEG_MASK_COUNTS 2
int ldmseg_loss_weight_mask(const void* src, int src_dtype, int B, int Hi, int Wi, int h, int w, int mode, int64_t ignore_label,
                            float* out, int32_t* flag, void* stream);
/* minmax[0] = x.min(), minmax[1] = x.max() of n fp32 values, on the device (NaN if x holds one, like torch).  scratch:
 * LDMSEG_MINMAX_SCRATCH_BYTES of device memory.  Two launches: per-workgroup partials, then one fixed-order finish. */
#define LDMSEG_MINMAX_SCRATCH_BYTES 3072
int ldmseg_tensor_minmax(const float* x, size_t n, float* minmax, void* scratch, void* stream);

/* ---- seg-VAE stage-1 loss: point CE, mask and KL terms (trainers_ae.py:204-216, losses.py:117-185, :303-394) ---------- */
#define LDMSEG_POINT_LOSS_MAX_C 128
/* present[b][c] = 1 where id c != ignore_label occurs in image b of targets [B,Ht,Wt] int64 once the pixels with valid == 0
 * (uint8 [B,Ht,Wt], may be NULL) count as ignore_label (losses.py:326; the caller's tensor is not written), else 0: what
 * prepare_targets (:397-439) finds with torch.unique.  Bit 0 of *flag (device int32) is set if an id other than ignore_label lies
 * outside [0, C).  Both outputs are reset by the call.  One launch; the caller reads the table once to size the draws. */
int ldmseg_class_presence(const int64_t* targets, const uint8_t* valid, int B, int Ht, int Wt, int C, int64_t ignore_label,
                          uint8_t* present, int32_t* flag, void* stream);
/* SegmentationLosses.point_loss (:364-394) without the matcher, forward only, on fp32 NCHW logits x [B,C,H,W] and targets / valid
 * as above.  Rows: B cross-entropy rows (one per image), then N mask rows; mask_rows_dev [N] int32 holds b * C + c of each object
 * mask, by image, then ascending class id (the order of prepare_targets).  Draws (device fp32 in [0, 1), [...,0] = x, [...,1] = y):
 * ce_over [B,S,2], ce_fresh [B,P-kU,2], mask_over [N,S,2], mask_fresh [N,P-kU,2]; S = int(P * oversample_ratio), kU =
 * int(importance_sample_ratio * P).  S == kU == 0 is oversample_ratio 0: the P fresh points serve directly (:164-165, :338-339).
 *   uncertainty  per oversampled point: CE rows second - first of the top two bilinear samples over the C channels (:296-301),
 *                mask rows -|bilinear sample of x[b,c]| (:294); the taps are those of F.grid_sample(align_corners=False, zeros
 *                padding) (csrc/point_sample.h).
 *   selection    exact top-kU of the S uncertainties of each row (radix select on the bit patterns); ties at the threshold go to
 *                the lower index (torch.topk defines no rule).  selected (may be NULL): int32 [B+N,kU], ascending per row.
 *   out[0]       ce: mean over the kept points of the batch of logsumexp(x / temperature) - x[label] / temperature at the kU
 *                selected + P-kU fresh points; label = nearest tap of the effective targets (0 outside the map), points with
 *                label == ignore_label are dropped; NaN if none is kept, like F.cross_entropy.
 *   out[1]       sum over mask rows of mean_P(binary_cross_entropy_with_logits(x, t)) / num_masks, t = bilinear sample of
 *                (effective target == c);  out[2]: sum of 1 - (2 sum(sigmoid(x) t) + 1) / (sum(sigmoid(x)) + sum(t) + 1) / num_masks.
 *                loss_masks (:117-185) returns out[1] + out[2].  N == 0: both 0.
 * Partial sums are fp64, stored per workgroup and added by one finishing launch in a fixed order: no float atomics, two calls on
 * the same inputs agree bit for bit.  scratch: ldmseg_point_loss_scratch_bytes(B + N, S, kU, P) bytes of device memory.  4 launches
 * (2 with kU == 0); no host synchronisation, no allocation. */
size_t ldmseg_point_loss_scratch_bytes(int rows, int S, int kU, int P);
int ldmseg_point_loss(const float* x, int B, int C, int H, int W, const int64_t* targets, const uint8_t* valid, int Ht, int Wt,
                      const int32_t* mask_rows_dev, int N, const float* ce_over, const float* ce_fresh, const float* mask_over,
                      const float* mask_fresh, int S, int kU, int P, int64_t ignore_label, float temperature, double num_masks,
                      float* out, int32_t* selected, void* scratch, void* stream);
/* DiagonalGaussianDistribution.kl() (vae.py:416-417) on moments [B, 2 * latent_channels, HW] (mean | logvar, logvar clamped to
 * [-30, 20]): per_image[b] = 0.5 * sum(mean^2 + exp(logvar) - 1 - logvar), added in fp64; mean (may be NULL) = their batch mean. */
int ldmseg_gaussian_kl(const float* moments, int B, int latent_channels, int HW, float* per_image, float* mean, void* stream);
/* Backward of ldmseg_point_loss to the logits: grad_x [B,C,H,W] = grad_ce * d ce / d x + grad_mask * d (out[1] + out[2]) / d x for
 * the call that had these arguments and returned `selected` (int32 [B+N,kU]; may be NULL only when kU == 0).  Coordinates, the
 * selection, the labels and the targets carry no gradient (the reference computes them under no_grad); the one differentiable path
 * is the bilinear sample of x at the chosen points.  grad_ce_dev / grad_mask_dev: device fp32 scalars; NULL = 0, and that term's
 * rows are then not evaluated at all.
 *   ce    point p of image b: (softmax_c(x_p / T) - [c == label_p]) / (T * K), K = kept points of the batch; dropped points give 0,
 *         and K == 0 gives 0 everywhere (the forward's ce is NaN there).
 *   mask  row (b, c), s = sigmoid(l), I = sum s t, D = sum s + sum t:
 *         ((s - t) / P - (2 t (D + 1) - (2 I + 1)) / (D + 1)^2 * s (1 - s)) / num_masks.
 * Each point gradient reaches grad_x[b, c] through its (up to four) taps inside the map.  No float atomics: every tap is stored
 * once into a per-pixel list (integer atomics count and place them), each list is ordered by (row, point, tap), and one pass over
 * the pixels adds every list in that order - two calls on the same inputs agree bit for bit.  grad_x is written completely (0.0
 * where no tap lands); the caller clears nothing.  scratch: ldmseg_point_loss_backward_scratch_bytes(...) bytes of device memory
 * (0 for sizes the call would refuse).  4 launches and one memset on `stream`; no host synchronisation, no allocation. */
size_t ldmseg_point_loss_backward_scratch_bytes(int B, int C, int H, int W, int N, int kU, int P);
int ldmseg_point_loss_backward(const float* x, int B, int C, int H, int W, const int64_t* targets, const uint8_t* valid, int Ht,
                               int Wt, const int32_t* mask_rows_dev, int N, const float* ce_over, const float* ce_fresh,
                               const float* mask_over, const float* mask_fresh, const int32_t* selected, int S, int kU, int P,
                               int64_t ignore_label, float temperature, double num_masks, const float* grad_ce_dev,
                               const float* grad_mask_dev, float* grad_x, void* scratch, void* stream);
/* Backward of ldmseg_gaussian_kl: grad_moments [B, 2 * latent_channels, HW] = grad_per_image[b] * (mean | 0.5 * (exp(logvar) - 1)
 * where -30 <= logvar <= 20, else 0) - the clamp passes gradient at its bounds, like torch.clamp.  One elementwise launch. */
int ldmseg_gaussian_kl_backward(const float* moments, int B, int latent_channels, int HW, const float* grad_per_image_dev,
                                float* grad_moments, void* stream);

/* ---- weight update: gradient-norm clipping + AdamW over a list of tensors (optim.py, trainers_ae.py:305-325) ------------ */
/* The list: n fp32 device tensors of numels[i] >= 0 elements each, at any 4-byte aligned address (16-byte loads and stores are
 * used where a tensor's addresses allow, scalar ones at its head and tail).  A tensor whose grads[i] is NULL is skipped wholly -
 * it does not enter the norm, its moments and parameter are not touched, its hyper entry is not read - which is torch's rule for a
 * parameter without .grad; numels[i] == 0 is allowed.
 *   norm pass    each workgroup squares and adds one chunk of one tensor in fp64 and stores one partial per chunk; the partials
 *                are then added in one fixed order.  No float atomics: two calls on the same inputs agree bit for bit, and the
 *                three entries below give the same norm bits for the same gradients.
 *   total_norm   (float)sqrt(sum): what clip_grad_norm_(..., norm_type=2) returns, up to the summation order.
 *   clipping     coef = min(1.0f, max_norm / (total_norm + 1e-6f)) in fp32; grads[i] *= coef is stored back, so that the gradients
 *                afterwards are what clip_grad_norm_ leaves (with coef == 1 the same bits).
 *   AdamW        per element, every operation rounded separately to fp32, in torch.optim.AdamW's order:
 *                  p = p * (1 - lr * wd);  m = m + (g - m) * (1 - beta1);  v = v * beta2 + (g * g) * (1 - beta2);
 *                  p = p - step_size * (m / (sqrt(v) / bc2_sqrt + eps)),
 *                step_size = lr / (1 - beta1^step) and bc2_sqrt = sqrt(1 - beta2^step) computed on the host in double, per
 *                tensor.  hyper[i].step is the count AFTER this update (>= 1); the caller keeps the counts.
 * scratch: ldmseg_multi_tensor_scratch_bytes(n, numels) bytes of device memory (0 for arguments the calls would refuse), owned by
 * the caller, reusable by a later call on the same stream.  Pointers and per-tensor scalars travel in the kernel arguments, at
 * most LDMSEG_MULTI_TENSOR_PER_LAUNCH tensors per launch: a list up to that length takes one launch per pass (ldmseg_grad_norm
 * one more, for the result), longer lists ceil(n / LDMSEG_MULTI_TENSOR_PER_LAUNCH) per pass plus one that adds the partials.
 * No host-device copy, no host synchronisation, no allocation.  LDMSEG_E_ARG: a null array, a negative numel, a pointer that is
 * not 4-byte aligned, a null parameter / moment of a tensor that is not skipped, step < 1, a beta outside [0, 1), a negative or
 * non-finite lr / eps / weight_decay, clipping (max_norm > 0) without total_norm_dev or scratch. */
#define LDMSEG_MULTI_TENSOR_PER_LAUNCH 48
typedef struct {
  double lr, beta1, beta2, eps, weight_decay;
  int64_t step;                  /* the count AFTER this update, >= 1 */
} ldmseg_adamw_hyper;
size_t ldmseg_multi_tensor_scratch_bytes(int n, const int64_t* numels);
/* total_norm_dev[0] = the L2 norm of all gradients of the list (0 for an empty one) */
int ldmseg_grad_norm(int n, const float* const* grads, const int64_t* numels, float* total_norm_dev, void* scratch, void* stream);
/* clip_grad_norm_(grads, max_norm): the norm to total_norm_dev, the gradients scaled in place.  max_norm must be positive. */
int ldmseg_grad_clip(int n, float* const* grads, const int64_t* numels, float max_norm, float* total_norm_dev, void* scratch,
                     void* stream);
/* clip (max_norm > 0; with max_norm <= 0 the norm pass is skipped, the gradients are not written and total_norm_dev may be NULL)
 * and one AdamW update of every tensor.  hyper: n entries on the host. */
int ldmseg_adamw_step(int n, float* const* params, float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                      const int64_t* numels, const ldmseg_adamw_hyper* hyper, float max_norm, float* total_norm_dev, void* scratch,
                      void* stream);

/* ---- sampler: TrainerDiffusion.sample (trainers_ldm_cond.py:1045-1170) -------------------- */
typedef struct {
  int32_t n_steps;               /* len(scheduler.timesteps) */
  const int64_t* timesteps;      /* host, descending */
  const float* coef;             /* host [n_steps][4]: sqrt_a_t, sqrt_b_t, sqrt_a_prev, sqrt_b_prev */
  int32_t prediction_type, clip_sample, self_condition;
  float clip_sample_range;
  /* build-defined mask inpainting (absent from the reference): all NULL = off */
  const uint8_t* known_dev;      /* [B,1,L,L] 1 = latent given */
  const float* z0_dev;           /* [B,4,L,L] scaled known latents */
  const float* noise_dev;        /* [B,4,L,L] the fixed noise draw */
  const float* paste_coef;       /* host [n_steps][2]: sqrt_a, sqrt_b of the NEXT timestep (last: 1,0) */
} ldmseg_sample_cfg;
/* Runs the whole loop on `stream`: latents [B,4,L,L] holds the initial noise on entry and the
 * final latents on exit (last step = pred_original_sample, :1154-1156).  If all_latents is
 * non-NULL it receives every step's latents [n_steps][B,4,L,L] (return_all_latents).
 * Separate-encoder handles: the image branch reads rgb_latents and timestep_img = 0 only (sample() passes no timestep_img,
 * trainers_ldm_cond.py:1141), so the loop computes its 12 residuals once, in step 0, into handle-owned memory
 * (B * 6,635,520 * (L/64)^2 elements of the compute dtype's storage, sized by ldmseg_unet_reserve) and every step adds them to
 * its skip connections in one launch; inpainting included.  Every call computes them again (the caller may have changed
 * rgb_latents).  ldmseg_debug_set(25, 1) makes every step compute them, the form the reference runs. */
int ldmseg_sample_loop(ldmseg_unet* h, const ldmseg_sample_cfg* cfg, float* latents, const float* rgb_latents,
                       int B, int L, float* all_latents, void* stream);
/* The sampling loop of a cross-attention handle with classifier-free guidance (trainers_ldm_cond.py:1098-1160); the plain
 * loop above returns LDMSEG_E_ARG on such a handle.  latents / rgb_latents / all_latents as there, B images.
 *   multiplier 2: ctx is [2B, S, ctx_dim], uncond half first; the UNet runs on cat([latents]*2) / cat([rgb]*2) (2B images),
 *                 then noise_pred = uncond + guidance_scale * (cond - uncond), each of the three fp32 ops rounded on its own
 *                 (torch's order), and the DDIM step runs on B images (last step: pred_original_sample).
 *   multiplier 1: ctx is [B, S, ctx_dim]; the model output is used as it is (guidance_scale ignored).
 * The context's keys / values are computed once per call (first step).  LDMSEG_E_ARG for self_condition with multiplier 2
 * (the reference fails at step 2 there), for the inpainting fields, on a separate-encoder handle (it has no cross-attention),
 * and as ldmseg_unet_forward_ctx for the context. */
int ldmseg_sample_loop_guided(ldmseg_unet* h, const ldmseg_sample_cfg* cfg, float* latents, const float* rgb_latents, int B, int L,
                              const float* ctx, int S, int ctx_dim, int multiplier, float guidance_scale, float* all_latents,
                              void* stream);

/* ---- bit codec of segment ids: COCO.encode_bitmap / decode_bitmap (ldmseg/data/coco.py:377-390) ---- */
/* ids [B,HW] int64 -> bits [B,n_bits,HW] fp32 (LSB first; ids == ignore_label -> fill_value), then *mul+add
 * (mul=2, add=-1 gives the seg-VAE input of trainers_ldm_cond.py:369); ignore_mask [B,HW] u8 may be NULL. */
int ldmseg_bit_encode(const int64_t* ids, int B, int n_bits, int HW, int64_t ignore_label, float fill_value, float mul,
                      float add, float* bits, uint8_t* ignore_mask, void* stream);
/* x [B,n_bits,HW] fp32 -> ids [B,HW] int64: bit k set iff x[:,k] > 0 */
int ldmseg_bit_decode(const float* x, int B, int n_bits, int HW, int64_t* ids, void* stream);

/* ---- diagnostics --------------------------------------------------------------------------- */
const char* ldmseg_last_error(void);
const char* ldmseg_version(void);
/* Kernel-family timing (HIP events on the launch stream).  enable=1 records an event pair
 * around every launch of the family (0 igemm, 1 attention, 2 groupnorm, 3 layernorm, 4 other);
 * ldmseg_profile_read synchronises the recorded events and returns launches / total ms /
 * algorithmic FLOPs and bytes since the last reset. */
int ldmseg_profile_enable(int enable);
int ldmseg_profile_read(int family, int64_t* launches, double* total_ms, double* flops, double* bytes);
int ldmseg_profile_reset(void);
/* one CSV line per recorded launch (family,label,ms,flops); label carries the launch shape */
int ldmseg_profile_dump(const char* path);
/* measurement knobs (defaults = the shipped configuration): key 1 = igemm tile-policy bits in value[8..12] (and, in
 * -DLDMSEG_IGEMM_ABLATE builds only, phase-ablation flags in value[0..7]); key 2 = attention query-tile choice;
 * keys 3/4 = low/high half of a device buffer for per-workgroup s_memtime stamps (ablate builds); key 5 = run every
 * igemm launch with that entry of the instantiation list (-1 = off; the launch table and the shape rules are bypassed -
 * tools/tune_igemm.py); keys 6/7 = ldmseg_bench_igemm only: number of weight copies the timing loop rotates over, and
 * whether the timed launch carries a folded LayerNorm; key 8 = GroupNorm kernel choice (0 = shipped, bit 0 = two-launch
 * scheme everywhere, bit 1 = cooperative kernel from 16x16 maps up, bit 2 = two-pass instead of one-pass small-map kernel, bit 5 (round 6) = no
 * one-workgroup-per-(image, group) kernel on the 16x16 / 32x32 maps); key 9 = K order of 3x3 conv launches: -1 = shipped
 * rule (channel-major on large maps with many input channels), 0 = (tap, channel) everywhere, 1 = (channel tile, tap,
 * channel) wherever the layer holds that packing; key 10 = cooperative GroupNorm hand-off: 1 = every workgroup computes
 * its partners' statistics itself instead of waiting for them (the path a workgroup takes when its partners are not
 * co-resident; results are bit-identical), 0 = shipped; key 11 = bound of the partner poll in microseconds (default 100);
 * key 12 = row-local fusion of the 320-channel transformer feed-forward (bit 0: LayerNorm_3 -> GEGLU -> ff.net.2, bit 1: +
 * proj_out; default 3, 0 = the unfused launches); key 13 bit 8 = no start-chunk rotation in that kernel; key 14 = step tail
 * (bit 0: dedicated conv_out kernel in bf16, bit 1: the sampling loop's scheduler step / self-condition / next-input pack in
 * its epilogue; default 3); key 15 = fp8 attention on the block-scaled 2x-rate MFMAs where the shape allows (head dim 40,
 * tokens a multiple of 128; default 1, 0 = the unscaled fp8 MFMAs of attention_fp8.hip; 0x111 = scaled MFMAs with exp +
 * convert instead of the direct e4m3 byte - attention_mx.hip); key 16 = row-local fusion of the 320-channel transformer entry
 * (proj_in -> LayerNorm_1 -> q|k|v in one launch, tproj.hip; bit 0 on, bit 1 loader block rotation; default 3, 0 = the unfused
 * launches); key 2 values: 0 = shipped rule, 7 = the round-3 rule (attention3.hip at head dim 40), 11..14 = attention4.hip forced
 * (8 / 4 waves, lazily tracked / every-tile maxima) - DESIGN 3.2 has every value of keys 2 and 15 as a table, csrc/attn_plan.h is
 * the rule; (key 17 was round 5's weight-streaming kernel - measured level with
 * igemm_kernel, now a record under tools/experiments/);
 * key 19 = resnet conv2 + conv_shortcut as one launch with an extra centre tap (bf16; default 1, 0 = two launches);
 * key 20 = ff.net.2 and proj_out of the 640- / 1280-channel transformers as one chained Linear over [g | h] (bf16; default 1);
 * key 21 = upsampler convs (nearest x2 -> conv3x3) as four 2x2-tap phase convs on the low-resolution map (bf16; default 1);
 * key 22 = the GroupNorm in front of a 320-channel transformer as a statistics pass + a sweep over the fused entry's LDS tile
 * (tproj.hip; bf16, maps of a multiple of 128 pixels; default 1, 0 = a GroupNorm launch of its own, n > 1 = n <= 64 pixel chunks);
 * key 23 (round 6) = K-sliced bf16 igemm launches reduce their slabs inside the launch when every (tile, slice) item has a
 * co-resident workgroup: bit 0 on for the 256-row tile forms (where it measured 2-4 % faster than slabs + a finish launch), bit 3 on
 * for every tile form that has the instantiation (measured 2-20 % slower on the 128-row tiles with 8 slices), bit 1 zero-length
 * partner poll (every workgroup but a tile's last arriver gives up at once and the last arriver reduces their shares - the path that
 * needs no co-residency; results are bit-identical), bit 2 = resnet conv1 -> norm2 on the maps whose conv runs on those tiles as
 * conv (finished in-launch) + GroupNorm instead of slabs + the fused finish-GroupNorm launch (moves where bf16 rounding happens, as on
 * the maps whose convs are not K-sliced), bits 8-23 = poll bound in microseconds (0 = 200); default 5, 0 = slabs + finish launches
 * everywhere.  Bits 0 / 1 / 3 never change a result bit;
 * key 24 = tuning: every plain-store igemm launch runs entry (v & 0xff) of the instantiation list with (v >> 8) K slices as if the
 * launch table held that entry (-1 = off; unlike key 5 the extra-tap / phase-conv routes stay);
 * key 25 = separate-encoder handles in ldmseg_sample_loop: 0 (default) the image branch runs once per call, 1 in every step
 * (the reference's form; results are bit-identical);
 * key 26 = weight gradient (ldmseg_vae_decode_backward / _encode_backward, ldmseg_op_conv*_wgrad*): the CU count handed to the
 * launch chooser, 0 (default; values below 0 count as 0) = the device's.  A count below the item count makes every workgroup walk
 * several (tile, slice) items - the path a smaller device or partition takes; the slicing, the scratch and every result bit stay
 * what they are (csrc/wgrad_plan.h; tests). */
int ldmseg_debug_set(int key, int value);
/* current value of a knob (keys 1, 8, 9, 11, 12, 14, 15, 16, 19, 20, 21, 22, 23, 25, 26); key -1 = the shipped default of key 1.  Tests restore through this, never a literal.
 * key 10 = number of cooperative-GroupNorm workgroups that took the self-computing path in ldmseg_op_* launches so far. */
int ldmseg_debug_get(int key);

#ifdef __cplusplus
}
#endif
#endif /* LDMSEG_HIP_H_ */
