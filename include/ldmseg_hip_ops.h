/* ldmseg_hip_ops.h - single-operator entry points of libldmseg_hip.so (fp32 boundary).
 *
 * Test support, not a product surface: tests/ drives each gfx950 kernel in isolation
 * through these and compares with the torch-CPU op the reference executes at that
 * point.  `dtype` is LDMSEG_F32 | LDMSEG_BF16 (the kernel's
 * compute/storage type); all tensors are fp32 device pointers; every call allocates
 * and frees its own staging buffers and is therefore slow.
 */
#ifndef LDMSEG_HIP_OPS_H_
#define LDMSEG_HIP_OPS_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* F.conv2d(cat([x, x2],1) [after nearest x2 upsample if up], w, bias, stride, padding=k/2); k in {1,3}.
 * ResnetBlock2D.conv1/conv2/conv_shortcut, Downsample2D, Upsample2D, proj_in/out (diffusers 0.16.1).
 * dtype 0 fp32, 1 bf16, 2 / 3 split-bf16 products on fp32 tensors (3: weights pre-split into hi | lo planes, as the bf16x3 handles). */
int ldmseg_op_conv2d(const float* x, const float* x2, const float* w, const float* bias, int B, int Ci, int Ci2, int H,
                     int W, int Co, int k, int stride, int up, int dtype, float* out, void* stream);
/* F.linear (+row bias per image, +residual, SiLU) or the GEGLU feed-forward half when geglu=1 */
int ldmseg_op_linear(const float* x, const float* w, const float* bias, const float* resid, const float* rowbias,
                     int rows_per_image, int M, int K, int N, int geglu, int silu, int splits, int dtype, float* out,
                     void* stream);
/* out = proj_out(h + ff.net.2(g)) + x - the end of a diffusers BasicTransformerBlock inside Transformer2DModel
 * (/root/reference/ldmseg/models/unet.py:401-425) - as the engines launch it at the 640- / 1280-channel levels: the chained matrix
 * [Wp W2 | Wp] and bias bp + Wp b2 formed once in fp32 (launch_chain_weights, the create-time kernel), then ONE Linear over [g | h]
 * with x as the residual.  g [M][4C], h / x / out [M][C], w2 [C][4C], wp [C][C]; b2 / bp may be NULL; C a multiple of 160. */
int ldmseg_op_chained_ff_out(const float* g, const float* h, const float* x, const float* w2, const float* b2, const float* wp,
                             const float* bp, int M, int C, int rows_per_image, int dtype, float* out, void* stream);
/* F.group_norm(cat([x,x2],1), 32, gamma, beta, eps) [+SiLU] */
int ldmseg_op_groupnorm(const float* x, const float* x2, const float* gamma, const float* beta, int B, int C, int C2,
                        int HW, float eps, int silu, int dtype, float* out, void* stream);
/* out = a + b on n_segs (<= 12) tensors in one launch, as the engine adds the separate image encoder's residuals to the skip
 * connections (skipadd.hip).  a / b / out: fp32 device arrays holding the segments back to back, each followed by
 * 8 guard elements (segment k starts at sum_{j<k} (seg_elems[j] + 8)); seg_elems on the HOST.  The operands are converted to the
 * storage type of `dtype` (0 fp32 | 1 bf16), the guard elements of the staging output are taken from `out` as it comes in, and the
 * whole staging output - guards included - is converted back into `out`: a guard that changed shows a write past a segment's end.
 * A segment that does not start 16-byte aligned in the staging buffers (after one of odd length) runs the kernel's
 * element-wise path. */
int ldmseg_op_skip_add(const float* a, const float* b, const int64_t* seg_elems, int n_segs, int dtype, float* out, void* stream);
/* F.layer_norm over the last dim [+SiLU] (also vae.py:309-322 LayerNorm2d in NHWC) */
int ldmseg_op_layernorm(const float* x, const float* gamma, const float* beta, int M, int C, float eps, int silu,
                        int dtype, float* out, void* stream);
/* diffusers Attention core on fused qkv [B,N,3C] -> [B,N,C] */
int ldmseg_op_attention(const float* qkv, int B, int N, int C, int heads, int dtype, float* out, void* stream);
/* the same under a causal mask (key j contributes to query i iff j <= i, built in the kernel from the indices): the attention
 * of transformers' CLIPTextModel.  Head dim 64 only (C == 64 * heads), any N >= 1; dtype 0 / 1 / 2 */
int ldmseg_op_attention_causal(const float* qkv, int B, int N, int C, int heads, int dtype, float* out, void* stream);
/* cross-attention core (diffusers Attention with a context, attn2): q [B,N,C], kv = to_k | to_v of the context [B,S,2C]
 * (channel = head*d + i), heads 8 -> out [B,N,C]; any S >= 1, d = C / heads in {40, 80, 160}; dtype 0 / 1 / 2 */
int ldmseg_op_attention_cross(const float* q, const float* kv, int B, int N, int S, int C, int heads, int dtype, float* out,
                              void* stream);
/* the same on the fp8 (e4m3) operand path of the bf16 mode (K/V pre-quantised, Q and P quantised in the kernel, fp32
 * accumulation; head dim 40 or 80) - BASELINE configs[4].  time_iters > 0 additionally times that many launches (pre-pass
 * + kernel) into *us_per_launch; out may be NULL then. */
int ldmseg_op_attention_fp8(const float* qkv, int B, int N, int C, int heads, float* out, int time_iters, float* us_per_launch,
                            void* stream);
/* nn.ConvTranspose2d(Ci, Co, kernel_size=2, stride=2)  (vae.py:154); dtype 0 / 1 / 2 / 3 as ldmseg_op_conv2d */
int ldmseg_op_convt2(const float* x, const float* w, const float* bias, int B, int Ci, int H, int W, int Co, int dtype,
                     float* out, void* stream);
/* The launch forms of the two VAEs (csrc/vae.hip), filled the way the models fill them; dtype as ldmseg_op_conv2d (0 / 1 / 2 / 3).
 * _vae_conv: one conv as Exec::conv and the VAE heads launch it.  pad -1 = padding k/2; pad 0 (k 3, stride 2 only) =
 * F.conv2d(F.pad(x, (0,1,0,1)), w, bias, stride=2), Ho = H / 2 (diffusers Downsample2D(padding=0) of AutoencoderKL).  epi 0: the
 * store epilogue, + resid [B,Co,Ho,Wo], then SiLU; n_store > Co stores explicit zero channels up to n_store as the seg-VAE encoder
 * does below a K tile (out still receives the Co real ones).  epi 2: fp32 NCHW straight from the launch (moments / logits heads;
 * no resid, no SiLU). */
int ldmseg_op_vae_conv(const float* x, const float* w, const float* bias, const float* resid, int B, int Ci, int H, int W, int Co, int k,
                       int stride, int pad, int silu, int epi, int n_store, int dtype, float* out, void* stream);
/* out [M,N] = a [M,K] @ b [N,K]^T (+ bias [N]) with an activation tensor as the weight operand (the three GEMMs of the image VAE's
 * single-head attention: Q K^T, W_v X^T, P V + b_v).  rows_f32 != 0: fp32 rows whatever the compute dtype (the scores).  dtype 2 / 3:
 * both operands are split in the K loop.  K a multiple of 64 (bf16) / 32, N of 32. */
int ldmseg_op_gemm_dynamic(const float* a, const float* b, const float* bias, int M, int N, int K, int rows_f32, int dtype, float* out,
                           void* stream);
/* torch.softmax(scale * s, -1) of fp32 rows s [rows,n] stored in `dtype` (0 / 1), returned as fp32; scale > 0, n % 4 == 0 */
int ldmseg_op_softmax_rows(const float* s, int rows, int n, float scale, int dtype, float* out, void* stream);
/* The fused tail of ldmseg_vae_decode_argmax on given logits x [B,C,H,W]: y = F.interpolate(x, scale_factor=2, 'bilinear'),
 * ids = y.argmax(1) (ignore_label where the max-softmax probability < mask_th, if mask_th >= 0), prob = softmax(y, 1).max(1) or NULL
 * (trainers_ldm_cond.py:427-433).  dtype 0 / 1; C a multiple of 4 / 8. */
int ldmseg_op_bilinear2x_argmax(const float* x, int B, int C, int H, int W, float mask_th, int64_t ignore_label, int dtype, int64_t* ids,
                                float* prob, void* stream);
/* ldmseg_op_layernorm with the buffers named: inplace != 0 normalises the tensor where it lies (what the seg-VAE decoder does behind
 * each ConvTranspose2d), 0 writes a second buffer */
int ldmseg_op_layernorm_io(const float* x, const float* gamma, const float* beta, int M, int C, float eps, int silu, int inplace, int dtype,
                           float* out, void* stream);
/* F.interpolate(scale_factor=2, mode='bilinear', align_corners=False)  (vae.py:270) */
int ldmseg_op_bilinear2x(const float* x, int B, int C, int H, int W, int dtype, float* out, void* stream);

/* The fused evaluation tail of ldmseg_vae_decode_panoptic on a given decoder output x4 [B,C,H4,W4] (f32 NCHW, packed to
 * NHWC `dtype` first); host geometry arrays as there.  volume (optional, device): the resampled logits [C][h_b*w_b] of
 * image b at C * out_offsets[b] - lets a test compare the interpolation chain with F.interpolate o crop o F.interpolate. */
int ldmseg_op_panoptic_from_decoder(const float* x4, int B, int C, int H4, int W4, int dtype, int in_h, int in_w,
                                    const int32_t* crop_boxes, const int32_t* out_sizes, const int64_t* out_offsets,
                                    int threshold_output, int threshold_mode, float mask_th, int count_th, double overlap_th,
                                    int64_t ignore_label, int32_t* labels, int32_t* panoptic, uint8_t* keep, int32_t* counts,
                                    int32_t* mask_counts, float* volume, void* stream);

/* The fused mIoU tail of ldmseg_vae_decode_semseg on a given decoder output x4 [B,C,H4,W4] (f32 NCHW, packed to NHWC `dtype`
 * first; C <= 256, a multiple of 4 (f32) / 8 (bf16)).  volume (optional, device): the resampled logits [B][C][out_h*out_w] fp32 -
 * lets a test compare the resampling with F.interpolate(align_corners=True) (trainers_ae.py:754). */
int ldmseg_op_semseg_from_decoder(const float* x4, int B, int C, int H4, int W4, int dtype, int out_h, int out_w, float mask_th,
                                  int64_t ignore_label, const int64_t* targets, int64_t ignore_index, int num_classes,
                                  int64_t* preds, int64_t* counts, float* volume, void* stream);

/* Entry of a transformer on caller-supplied weights: h = x Wp^T + bp (proj_in, /root/reference/ldmseg/models/unet.py:361-373 via
 * diffusers Transformer2DModel), q|k|v = [Wq | Wk | Wv] LayerNorm(h; gamma, beta).  mode 0: unfused launches; 1: the row-local fused
 * kernel (bf16, C = 320, M % 128 == 0).  h_out [M][C], qkv_out [M][3C] fp32.  time_iters > 0 also times the chosen path. */
int ldmseg_op_transformer_in(const float* x, const float* wp, const float* bp, const float* gamma, const float* beta, const float* wq,
                             const float* wk, const float* wv, int M, int C, float eps, int dtype, int mode, float* h_out, float* qkv_out,
                             int time_iters, float* us_per_call, void* stream);
/* The same behind the transformer's GroupNorm (32 groups, eps gn_eps, no SiLU; diffusers Transformer2DModel.norm) over
 * x = [images][M / images][C] rows.  gn_mode 0: a GroupNorm launch, then the entry as above; gn_mode 1 (mode 1 only, M / images a
 * multiple of 128): the statistics pass alone, the normalisation applied to the row tile inside the fused kernel (tproj.hip). */
int ldmseg_op_gn_transformer_in(const float* x, const float* gn_gamma, const float* gn_beta, float gn_eps, int images, int gn_mode,
                                const float* wp, const float* bp, const float* gamma, const float* beta, const float* wq,
                                const float* wk, const float* wv, int M, int C, float eps, int dtype, int mode, float* h_out,
                                float* qkv_out, int time_iters, float* us_per_call, void* stream);

/* One conv / GEMM layer launched exactly as the engine launches it inside a forward (NHWC operands, the engine's
 * split-K plan when splits == 0, row-major store epilogue with bias / per-image bias row / residual / SiLU, or GEGLU):
 * F.conv2d(cat([x,x2],1) [nearest x2 if up], w, bias, stride, k/2) + rowbias[b,:,None,None] + resid, then SiLU;
 * geglu=1: w [Co,Ci] is ff.net.0.proj, out = a * gelu(gate) with [a | gate] = chunk(2, dim=1), Cout = Co/2.
 * NCHW f32 boundary like the other ops. */
int ldmseg_op_igemm(const float* x, const float* x2, const float* w, const float* bias, const float* resid,
                    const float* rowbias, int B, int Ci, int Ci2, int H, int W, int Co, int k, int stride, int up, int geglu,
                    int silu, int splits, int dtype, float* out, void* stream);
/* F.conv2d(h, w2, b2, padding=1) + F.conv2d(torch.cat([xs, xs2], 1), ws, bs): the tail of diffusers' ResnetBlock2D where
 * cin != cout (conv2 + conv_shortcut, ldmseg/models/unet.py:361-425 run them through diffusers 0.16.1's resnet.py) as the
 * engine's ONE bf16 launch with an extra centre tap.  xs2 NULL / Cs2 = 0 when the shortcut input is not a concat.  iters > 0
 * additionally times `iters` launches (us_per_launch).  -4: the shape has no such launch (the engine then runs two convs). */
int ldmseg_op_conv3x3_plus_1x1(const float* h, const float* w2, const float* b2, const float* xs, const float* xs2, const float* ws,
                               const float* bs, int B, int C, int Cs, int Cs2, int H, int W, int Co, int splits, int dtype, float* out,
                               int iters, float* us_per_launch, void* stream);
/* [silu](F.group_norm(F.conv2d(x, w, bias, padding=1) + rowbias[b,:,None,None], 32, gamma, beta, eps)) the way the engine runs
 * resnet conv1 -> norm2 on small maps: the conv as `splits` (>= 2) K slices, then ONE kernel that sums the slices, adds bias and
 * time-embedding row and normalises (launch_finish_groupnorm).  Returns -4 when the shape has no fused instantiation. */
int ldmseg_op_conv_groupnorm(const float* x, const float* w, const float* bias, const float* rowbias, const float* gamma,
                             const float* beta, int B, int Ci, int H, int W, int Co, float eps, int silu, int splits, int dtype,
                             float* out, void* stream);
/* F.linear(F.layer_norm(x, (K,), gamma, beta, eps), w, bias) - GEGLU on top when geglu=1 - the way the engine runs
 * norm1 -> to_q|k|v and norm3 -> ff.net.0.proj (diffusers BasicTransformerBlock): one statistics pass over x, then the GEMM on
 * the un-normalised x with gamma folded into the weights and rstd*(acc - mean*c1) + c2 in the epilogue.  Without GEGLU, an N
 * that is no multiple of 160 is padded with zero weight rows to the next one (the folded instantiations have 160-column tiles;
 * the CLIP vision executor pads its N = 3072 / 4096 the same way) in every dtype; GEGLU keeps its 128-column tile. */
int ldmseg_op_ln_linear(const float* x, const float* gamma, const float* beta, const float* w, const float* bias, int M, int K,
                        int N, float eps, int geglu, int dtype, float* out, void* stream);
/* silu(F.linear(F.layer_norm(x, (K,), gamma, beta, eps), w, bias)) launched the way the CLIP vision executor launches
 * layer_norm2 -> mlp.fc1 (transformers CLIPMLP with quick_gelu, whose x * sigmoid(1.702 x) the executor obtains from this SiLU
 * epilogue by scaling fc1 by 1.702 and fc2 by 1 / 1.702): the folded-LayerNorm GEMM with the SiLU flag of the store epilogue. */
int ldmseg_op_ln_linear_silu(const float* x, const float* gamma, const float* beta, const float* w, const float* bias, int M,
                             int K, int N, float eps, int dtype, float* out, void* stream);
/* The front kernel of the CLIP vision executor: F.unfold(x, P, stride=P) rows, k = (channel, dy, dx), of
 * x = (F.interpolate(img, (S,S), mode='bilinear', align_corners=False) - mean) / std (norm_resize_images, trainers_ldm_cond.py:
 * 663-675; resample = 0: x = img, already S x S) -> out [B * (S/P)^2][Kpad] fp32, Kpad = 3 P P rounded up to a multiple of 64,
 * zero beyond 3 P P.  mean / std: host arrays of 3. */
int ldmseg_op_clip_patch_rows(const float* img, int B, int H, int W, int S, int P, const float* mean, const float* std,
                              int resample, int dtype, float* out, void* stream);
/* the row-local kernels of the CLIP text executor (clip_text.hip).  _tokens: out[r][t] = tok[ids[r][t]] + pos[t], summed in
 * fp32 and rounded once to `dtype` (ids int64 [R, T], tok [vocab, C], pos [>= T, C], out [R * T, C] fp32 holding the rounded
 * values).  _final_ln: out = F.layer_norm(x, (C,), gamma, beta, eps) of every row of x [M, C] as stored in `dtype`. */
int ldmseg_op_clip_text_tokens(const int64_t* ids, const float* tok, const float* pos, int R, int T, int C, int vocab, int dtype,
                               float* out, void* stream);
int ldmseg_op_clip_text_final_ln(const float* x, const float* gamma, const float* beta, int M, int C, float eps, int dtype,
                                 float* out, void* stream);
/* The tail of a transformer block on [M, C] token rows (diffusers BasicTransformerBlock.ff + Transformer2DModel.proj_out,
 * /root/reference/ldmseg/models/unet.py:401-425):  h2 = h + ff.net.2(GEGLU(ff.net.0.proj(LayerNorm(h))));  out = proj_out(h2) + x.
 * mode 0 = the unfused launches, 1 = row-local fused feed-forward (tfuse.hip) + proj_out GEMM, 3 = all in the fused kernel
 * (modes 1 / 3: bf16, C = 320).  time_iters > 0: *us_per_call = average microseconds of the whole tail. */
int ldmseg_op_transformer_ff(const float* h, const float* x, const float* gamma, const float* beta, const float* w1, const float* b1,
                             const float* w2, const float* b2, const float* wp, const float* bp, int M, int C, float eps, int dtype,
                             int mode, float* out, int time_iters, float* us_per_call, void* stream);
/* The step-tail kernel (tail.hip, bf16): eps = conv_out(x) (3x3, 320 -> 4, /root/reference/ldmseg/models/unet.py:433-436) and,
 * with ddim != 0, DDIMNoiseScheduler.step (ddim_scheduler.py:231-267) on `latents` in place (last: pred_original_sample), the
 * inpainting paste, the self-condition write (trainers_ldm_cond.py:1151-1159) and the next step's packed input
 * [latents | rgb | cond | 0] as fp32 [B, H*W, 64].  coef4 is a HOST array; eps_out / cond / known / xin_out may be NULL. */
int ldmseg_op_conv_out_tail(const float* x, const float* w, const float* bias, int B, int H, int W, float* eps_out, int ddim, int last,
                            const float* coef4, int pred_type, int clip, float clip_range, float* latents, float* cond,
                            const float* rgb, const uint8_t* known, const float* z0, const float* noise, float sa, float sb,
                            float* xin_out, void* stream);
/* Kernel timing for tuning (tools/kbench.py): the same launches repeated `iters` times back to back on `stream` between
 * two HIP events; *us_per_launch = average microseconds (igemm: including the split-K finish kernel if the plan has one). */
int ldmseg_bench_igemm(const float* x, const float* x2, const float* w, const float* bias, const float* resid,
                       const float* rowbias, int B, int Ci, int Ci2, int H, int W, int Co, int k, int stride, int up, int geglu,
                       int silu, int splits, int dtype, int iters, float* us_per_launch, void* stream);
int ldmseg_bench_groupnorm(const float* gamma, const float* beta, int B, int C, int C2, int HW, int silu, int dtype, int iters,
                           float* us_per_launch, void* stream);
int ldmseg_bench_attention(const float* qkv, int B, int N, int C, int heads, int dtype, int iters, float* us_per_launch,
                           void* stream);
/* "igemm<dtype,BM,BN,WM,WN,NST,PIPE,LDR> splits=S grid=G": template instantiation and plan of the most recent igemm
 * launch of this process - lets a parity test assert WHICH kernel it just compared with the oracle. */
int ldmseg_igemm_last_kernel(char* buf, int n);
/* The same string for a launch that is only described - what ldmseg_igemm_last_kernel would report after it, under the current
 * ldmseg_debug_set state, on a device of `cus` compute units.  No device is touched.  desc: 17 ints, M, N, C0, C1, C2, C3, taps,
 * stride, up, up4, cm, epi (0 store, 1 GEGLU), lnf (a LayerNorm is folded), x3, splits (0 = planned the way the engines plan the
 * K slices), no_finish, region (the caller has a counter region for the in-launch finish).  dtype 0 fp32, 1 bf16, 2 / 3 = fp32
 * with x3 = 1 / 2 as the operators take it.  Returns 0, or -2 when the library has no such launch. */
int ldmseg_op_igemm_plan(const int* desc, int dtype, int cus, char* buf, int n);
/* What ldmseg_op_groupnorm would launch for (B, C + C2 channels in `groups` groups, HW pixels) on a device with `cus` compute units,
 * under the current debug knobs (keys 8, 10, 11); needs no device.  region_ok: a hand-off region for the cooperative kernel
 * exists.  buf receives the dispatch-log names joined by " + " and " splits=S grid=GXxGY block=T" (two launches:
 * grid=GXxGY+GXxGY).  Returns 0, or -2 where ldmseg_op_groupnorm returns -2.  ldmseg_op_conv_groupnorm_plan: the finish +
 * GroupNorm launch of ldmseg_op_conv_groupnorm over Co channels; -4 where that returns -4. */
int ldmseg_op_groupnorm_plan(int B, int C, int C2, int HW, int groups, int dtype, int cus, int region_ok, char* buf, int n);
int ldmseg_op_conv_groupnorm_plan(int B, int Co, int HW, int dtype, char* buf, int n);
/* What ldmseg_op_layernorm (stats = 0) or the row-statistics pass of ldmseg_op_ln_linear (stats = 1) would launch for M rows of C
 * channels under the current debug key 8 (csrc/ln_plan.h; needs no device).  buf receives "name grid=GX block=T" with the
 * dispatch-log name.  Returns 0, or -2 where the launch returns -2. */
int ldmseg_op_layernorm_plan(int M, int C, int dtype, int stats, char* buf, int n);
/* What an attention operator would launch under the current debug keys 2 and 15 (csrc/attn_plan.h; needs no device): kind 0 =
 * ldmseg_op_attention, 1 = ldmseg_op_attention_causal, 2 = ldmseg_op_attention_fp8 (dtype ignored), 3 = ldmseg_op_attention_cross
 * over S context rows (S is ignored otherwise).  buf receives, per launch, "name grid=GXxGY block=T" (the fp8 pre-passes and the
 * cross kernel, on 3-D grids: grid=GXxGYxGZ) with the dispatch-log name, the pre-pass of the fp8 forms first, joined by " + ".
 * Returns 0, or -2 where the operator returns -2. */
int ldmseg_op_attention_plan(int kind, int B, int N, int S, int C, int heads, int dtype, char* buf, int n);
/* enable=1 clears and starts a log of the DISTINCT igemm instantiations launched ("igemm<...>" + "/splitk" for K-sliced
 * launches; ",x3" / ",x3w" for split-bf16 products) and of the fused GEMM kernels; enable=2 logs every kernel of the UNet
 * forward path (split-K finish, GroupNorm, LayerNorm statistics, attention too), each named with its template arguments and
 * run-time form; enable=0 stops it; _read copies them newline-separated.  The parity suite uses it to prove that every
 * kernel a full-size forward runs is also compared with the oracle by a per-op test. */
int ldmseg_igemm_log(int enable);
int ldmseg_igemm_log_read(char* buf, int n);

/* The time-embedding path, which runs in fp32 in every compute mode and stays out of the dispatch log.  Nothing is staged: every
 * tensor is fp32 (timesteps int64) on the device already.
 * _time_sinusoid: out [B,320] = diffusers Timesteps(320, flip_sin_to_cos=True, freq_shift=0) = [cos(t f_i) | sin(t f_i)],
 *   f_i = exp(-ln(1e4) i / 160), of the timesteps given as a forward takes them: t_dev with t_count = B entries, or with t_count = 1
 *   entry for all B rows, or (t_dev NULL) t_host for all rows.  -2: B < 1, out NULL, t_dev with t_count not in {1, B}.
 * _small_linear: y [B,N] = act_out(F.linear(act_in(x [B,K]), W [N,K], bias [N] or NULL)), act = SiLU where its flag is set - the
 *   Linear of TimestepEmbedding, of every time_emb_proj and of the CLIP visual projection.  Any B >= 1.  -2: x, W or y NULL,
 *   B, K or N below 1.
 * _unet_time_rows: the handle's own time-embedding pass (the one function behind every forward and both sampling loops) for n
 *   timesteps (HOST array), the way the loops run it: linear_1 -> SiLU -> linear_2 -> time_emb_proj(SiLU(.)) of every resnet of
 *   table 0 (the UNet's resnets in model order) or 1 (down_blocks_additional of a separate-encoder handle), in chunks of 64 rows,
 *   into rows_dev [n, *total_out].  rows_dev NULL: only *total_out is set.  Any n >= 1; scratch memory of its own; waits for the
 *   stream.  -2: a NULL handle / timesteps / total_out, n < 1, a negative timestep, table 1 on another handle, any other table. */
struct ldmseg_unet;
int ldmseg_op_time_sinusoid(const int64_t* t_dev, int t_count, int64_t t_host, int B, float* out, void* stream);
int ldmseg_op_small_linear(const float* x, const float* W, const float* bias, int B, int K, int N, int silu_in, int silu_out, float* y,
                           void* stream);
int ldmseg_unet_time_rows(struct ldmseg_unet* h, const int64_t* timesteps_host, int n, int table, float* rows_dev, int* total_out,
                          void* stream);

/* The kernels of the seg-VAE decoder's backward (csrc/vae_bwd.hip), each by itself.  Every tensor is fp32 on the device;
 * dtype picks the products: 0 = fp32, 2 / 3 = split-bf16 (3: data-gradient weights as hi | lo planes, as a bf16x3 handle holds
 * them).  Gradients come back in the state-dict layout.  -2: a shape or dtype the kernels do not serve.
 * _conv_wgrad:   x [B,Ci,H,W], dy [B,Co,H,W] -> dw [Co,Ci,3,3], db [Co] or NULL of F.conv2d(x, w, b, padding=1).
 * _convt2_wgrad: x [B,Ci,H,W], dy [B,Co,2H,2W] -> dw [Ci,Co,2,2], db [Co] or NULL of F.conv_transpose2d(x, w, b, stride=2).
 * _conv_dgrad:   dy [B,Co,H,W], w [Co,Ci,3,3] -> dx [B,Ci,H,W] (igemm on the transposed, tap-rotated packing); nchw_epi = 1 stores
 *                through the fp32 NCHW epilogue, as the latents' gradient is stored.
 * _convt2_dgrad: dy [B,Co,2H,2W], w [Ci,Co,2,2] -> dx [B,Ci,H,W].
 * _groupnorm_silu_bwd: backward of silu(group_norm(x, 32, gamma, beta, eps)); x, dy, dx [B,C,HW]; dgamma / dbeta [C] or NULL.
 * _layernorm_silu_bwd: backward of silu(layer_norm(x, (C,), gamma, beta, eps)) over rows; x, dy, dx [M,C]; pm = 1: the rows are the
 *                pixels of maps H2 x W2 and dx is stored phase-major, [image][H2/2][W2/2][2x2][C], as the transposed-conv gradients
 *                read it.
 * _wgrad_plan:   what a weight-gradient launch of P pixels, N dY columns, C storage channels of X, taps 9 | 1 would run on a device
 *                of `cus` CUs (csrc/wgrad_plan.h; needs no device): "name tiles=T slices=S steps=K/TOTAL grid=G block=256 one_per_cu=0|1". */
int ldmseg_op_conv_wgrad(const float* x, const float* dy, int B, int Ci, int H, int W, int Co, int dtype, float* dw, float* db, void* stream);
int ldmseg_op_convt2_wgrad(const float* x, const float* dy, int B, int Ci, int H, int W, int Co, int dtype, float* dw, float* db, void* stream);
int ldmseg_op_conv_dgrad(const float* dy, const float* w, int B, int Ci, int H, int W, int Co, int nchw_epi, int dtype, float* dx, void* stream);
int ldmseg_op_convt2_dgrad(const float* dy, const float* w, int B, int Ci, int H, int W, int Co, int dtype, float* dx, void* stream);
int ldmseg_op_groupnorm_silu_bwd(const float* x, const float* dy, const float* gamma, const float* beta, int B, int C, int HW, float eps,
                                 float* dx, float* dgamma, float* dbeta, void* stream);
int ldmseg_op_layernorm_silu_bwd(const float* x, const float* dy, const float* gamma, const float* beta, int M, int C, float eps, int pm,
                                 int H2, int W2, float* dx, float* dgamma, float* dbeta, void* stream);
int ldmseg_op_wgrad_plan(int P, int N, int C, int taps, int x3, int cus, char* buf, int n);

/* What the seg-VAE encoder's backward adds; tensors and dtype as above.
 * _conv_wgrad_ex: _conv_wgrad of F.conv2d(x, w, b, stride=stride, padding=1), stride 1 | 2, on the tile the storage widths choose
 *                (32 | 64 | 128 rows of dY by 32 | 64 | 128 channels of X): x [B,Ci,H,W], dy [B,Co,Ho,Wo] with Ho = (H - 1) / stride + 1.
 * _conv_s2_wgrad: _conv_wgrad_ex with stride 2.
 * _conv_s2_dgrad: dy [B,Co,Ho,Wo], w [Co,Ci,3,3] -> dx [B,Ci,H,W] of F.conv2d(x, w, stride=2, padding=1): one igemm launch over dY
 *                whose 4 Ci columns are the four output phases of dX, scattered by the transposed conv's epilogue.  Ci a multiple of 4.
 * _silu_bwd:     du[i] = da[i] * silu'(u[i]) on n floats.  _silu_fwd: a[i] = silu(u[i]), the launch behind a SiLU-less conv there.
 * _wgrad_plan_ex: _wgrad_plan of the by-width rule, P = the pixels of the OUTPUT map, stride 1 | 2; macs_per_pixel (or NULL)
 *                receives tiles x tile area, the MACs the launch executes per pixel. */
int ldmseg_op_conv_wgrad_ex(const float* x, const float* dy, int B, int Ci, int H, int W, int Co, int stride, int dtype, float* dw, float* db,
                            void* stream);
int ldmseg_op_conv_s2_wgrad(const float* x, const float* dy, int B, int Ci, int H, int W, int Co, int dtype, float* dw, float* db, void* stream);
int ldmseg_op_conv_s2_dgrad(const float* dy, const float* w, int B, int Ci, int H, int W, int Co, int dtype, float* dx, void* stream);
int ldmseg_op_silu_bwd(const float* u, const float* da, int64_t n, float* du, void* stream);
int ldmseg_op_silu_fwd(const float* u, int64_t n, float* a, void* stream);
int ldmseg_op_wgrad_plan_ex(int P, int N, int C, int taps, int x3, int stride, int cus, char* buf, int n, int64_t* macs_per_pixel);

/* q[i] = n[i] / d (0 <= n[i] < 2^31, d >= 1) computed the way the kernels divide: host-prepared multiply-shift pair */
int ldmseg_op_fastdiv(const int* n, int count, int d, int* q, void* stream);

/* src[i], i in [0, out_size): the source index ldmseg_loss_weight_mask reads for output index i when it resizes in_size to
 * out_size (csrc/nearest_index.h, the rule of F.interpolate(mode='nearest')).  Host only: src is a host array, no GPU is touched. */
int ldmseg_op_nearest_index(int in_size, int out_size, int* src);

/* The taps ldmseg_point_loss reads for n points u [n,2] (u[...,0] = x, u[...,1] = y) of a [H,W] map: those of
 * F.grid_sample(input, 2 * u - 1, align_corners=False, padding_mode='zeros') (csrc/point_sample.h).  mode 0 bilinear: index [n,4]
 * (y * W + x of the north-west, north-east, south-west, south-east tap, -1 outside the map) and weight [n,4]; mode 1 nearest (half
 * to even): index [n], -1 outside the map, weight unused.  Host only: the arrays are host arrays, no GPU is touched. */
int ldmseg_op_point_taps(int n, const float* u, int H, int W, int mode, int32_t* index, float* weight);

#ifdef __cplusplus
}
#endif
#endif
