// Host-side launch API of the seg-VAE's backward kernels (vae_bwd.hip): the decoder's and what the encoder's adds
// (DESIGN 8.7).  Every tensor is fp32: the backward runs on fp32-storage handles only ("fp32" and "bf16x3"); x3 selects the
// split-bf16 products of the weight gradient.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "wgrad_plan.h"

namespace ldmseg {

// Weight gradient of a 3x3 conv (pad 1, stride 1; taps = 9) or of any GEMM over pixel rows (taps = 1):
//   slab[s][n][tap * C + c] = sum over the pixels p of slice s of dy[p][n] * x[p + tap][c]   (zero outside the image)
// dy [P][ldy] (the first N columns are taken, N <= ldy), x [P][C] on B maps of H x W pixels (P = B H W).  The slabs
// (wgrad_partial_bytes) are then added in slice order by the same call.
// stride 2 (taps 9): x lives on B maps of H x W, dy on the conv's output maps Ho x Wo (conv_out_dim of H and W), and
//   slab[s][n][tap * C + c] = sum over the OUTPUT pixels p = (oy, ox) of slice s of dy[p][n] * x[(2 oy + ty - 1, 2 ox + tx - 1)][c].
// rule: the decoder's fixed 128 x 128 tile, or the tile that follows the storage widths N and C (wgrad_plan.h).
struct WgradParams {
  const float* dy = nullptr; int ldy = 0;
  const float* x = nullptr;
  int B = 0, H = 0, W = 0;
  int N = 0, C = 0, taps = 9;
  int x3 = 0;
  float* partial = nullptr;
  int stride = 1;
  WgradRule rule = kWgradFixedTile;
};
// out = the slabs added in slice order, in the state-dict layout: form 0 = Conv2d [n_real][c_real][3][3] (taps 9) or Linear
// [n_real][c_real] (taps 1); form 1 = ConvTranspose2d k2 s2 [c_real][co][2][2] from rows n = q * co + o (taps 1, n_real = 4 co)
struct WgradOut { int form, n_real, c_real, co; float* out; };
int wgrad_plan(const WgradParams& p, int cus, WgradPlan* pl);
// The CU count the callers of wgrad_plan hand it: the device's, or what debug key 26 names (> 0; tests: a grid smaller than the
// item count, i.e. workgroups that walk several items).  The slicing does not depend on it, so neither do the scratch or the bits.
void wgrad_set_cus(int cus);          // <= 0: the device's
int wgrad_get_cus();                  // the override, 0 = none
int wgrad_cus();
size_t wgrad_partial_bytes(const WgradParams& p, const WgradPlan& pl);
// two launches: the plan's kernel (wgrad_plan_name) into the slabs, then wgrad_finish<conv | convt> into o.out
int launch_wgrad(const WgradParams& p, const WgradPlan& pl, const WgradOut& o, hipStream_t s);

// Row r = (image, Y, X) of maps H2 x W2 in phase-major order [image][H2/2][W2/2][2x2]: what launch_ln_silu_bwd stores with pm = 1
// and both transposed-conv gradients read.  R: the row index's type (int where the rows fit one).
template <typename R>
__host__ __device__ inline size_t phase_major_row(R r, int H2, int W2) {
  const int hw = H2 * W2;
  const int img = (int)(r / hw), rem = (int)(r - (R)img * hw);
  const int Y = rem / W2, X = rem - Y * W2;
  return (((size_t)img * (H2 >> 1) + (Y >> 1)) * (W2 >> 1) + (X >> 1)) * 4 + 2 * (Y & 1) + (X & 1);
}

// out[j] = sum_p a[p][q * qstride + j] over rows p and q < Q, for j < n: the bias gradient of a conv (Q = 1) or a transposed conv
// (Q = 4, qstride = Co).  Rows are cut into colsum_slices(P) runs whose sums (scratch: colsum_scratch_bytes) are added in order.
int colsum_slices(int P);
size_t colsum_scratch_bytes(int P, int N);
int launch_colsum(const float* a, int lda, int P, int N, int Q, int qstride, int n, float* scratch, float* out, hipStream_t s);

// LayerNorm over the last dim of [M][C] followed by SiLU, backward: x = the forward's INPUT, dy = d / d SiLU(LN(x)).  dx, dgamma,
// dbeta as DESIGN 8.6.  pm: dx row r = (image, Y, X) of a map H2 x W2 is stored phase-major, at row
// phase_major_row(r, H2, W2) - the [B, H, W, 2x2, C] order both transposed-conv gradients read.
// dgamma / dbeta null: not computed.  scratch: ln_bwd_scratch_bytes(M, C).  C a multiple of 64, at most 1024.
size_t ln_bwd_scratch_bytes(int M, int C);
int launch_ln_silu_bwd(const float* x, const float* dy, const float* gamma, const float* beta, float* dx, float* dgamma, float* dbeta,
                       int M, int C, float eps, int pm, int H2, int W2, float* scratch, hipStream_t s);

// GroupNorm (32 groups) + SiLU backward on [B][HW][C]; statistics are recomputed from x.  scratch: gn_bwd_scratch_bytes(B, C)
size_t gn_bwd_scratch_bytes(int B, int C);
int launch_gn_silu_bwd(const float* x, const float* dy, const float* gamma, const float* beta, float* dx, float* dgamma, float* dbeta,
                       int B, int HW, int C, float eps, float* scratch, hipStream_t s);

// du = da * silu'(u), elementwise on n floats (the four conv + SiLU layers of the encoder keep u); a = silu(u), its forward
int launch_silu_bwd(const float* u, const float* da, float* du, size_t n, hipStream_t s);
int launch_silu_fwd(const float* u, float* a, size_t n, hipStream_t s);

// z = mean + exp(0.5 clamp(logvar, -30, 20)) noise, backward to the moments [B][8][HW] = (mean | logvar): d mean = dz,
// d logvar = dz * noise * 0.5 * std where -30 <= logvar <= 20 and 0 elsewhere (noise null: zeros).  dz [B][4][HW] * scale.
int launch_posterior_backward(const float* moments, const float* noise, float scale, const float* dz, float* dmoments, int B, int HW,
                              hipStream_t s);

// Weights of the data gradients, read by launch_igemm as ordinary [Npad][K] fp32 matrices:
// Conv2d OIHW [Co][Ci][3][3] -> [Npad][9][Cop], row ci, column (tap', co) = w[co][ci][8 - tap'] (transposed, taps rotated by 180 degrees)
int launch_pack_dgrad_conv(const float* w, float* out, int Co, int Ci, int Npad, int Cop, hipStream_t s);
// Conv2d OIHW [Co][Ci][3][3] of a STRIDE-2 conv (pad 1) -> [Npad][9][Cop], row q * Ci + ci for the output phase q = 2 py + px of dX,
// column (tap', co) = w[co][ci][py + 3 - 2 ty'][px + 3 - 2 tx'] where that tap exists and zero elsewhere (tap' = (ty', tx') is the
// window position on dY, offsets ty' - 1): igemm over dY with EPI_CONVT2 then scatters row (y, x), column q * Ci + ci to
// dX[2 y + py][2 x + px][ci].  Npad >= 4 Ci.
int launch_pack_dgrad_conv_s2(const float* w, float* out, int Co, int Ci, int Npad, int Cop, hipStream_t s);
// ConvTranspose2d [Ci][Co][2][2] -> [Npad][4 Co], row ci, column q * Co + co = w[ci][co][q]
int launch_pack_dgrad_convt(const float* w, float* out, int Ci, int Co, int Npad, hipStream_t s);

// The shapes of those three packings as igemm takes them (the fields of the runtime's ConvW): N rows padded to the launch's N tile,
// n_valid real ones, K = taps * cin_pad.  The handles' packings and the ldmseg_op_*_dgrad operators are sized by them.
struct DgradShape { int N, n_valid, cin_pad, taps, cout; };
constexpr int kDgradKTile = 32;      // fp32 channels per 128-B K tile
inline int dgrad_pad(int n, int to) { return (n + to - 1) / to * to; }
// dX = conv3x3(dY, W transposed and rotated by 180 degrees): N = Ci, K = 9 * Co (Co padded to a K tile); epi: the launch's epilogue
inline DgradShape dgrad_conv_shape(int Co, int Ci, int epi) { return {dgrad_pad(Ci, igemm_pick_bn(Ci, epi)), Ci, dgrad_pad(Co, kDgradKTile), 9, Ci}; }
// dX of a STRIDE-2 conv3x3 = the four output phases as 4 Ci columns of one 3x3 GEMM over dY, scattered by EPI_CONVT2
inline DgradShape dgrad_conv_s2_shape(int Co, int Ci) {
  return {dgrad_pad(4 * Ci, igemm_pick_bn(4 * Ci, EPI_CONVT2)), 4 * Ci, dgrad_pad(Co, kDgradKTile), 9, Ci};
}
// dX[p] = dY[p, 2x2, :] W[ci][co][q]: N = Ci, K = 4 * Co on the phase-major dY
inline DgradShape dgrad_convt_shape(int Ci, int Co) { return {dgrad_pad(Ci, igemm_pick_bn(Ci, EPI_STORE)), Ci, 4 * Co, 1, Ci}; }

}  // namespace ldmseg
