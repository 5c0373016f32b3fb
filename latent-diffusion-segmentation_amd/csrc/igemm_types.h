// The plain-data types of the igemm launcher that every translation unit sees (kernels.h); the rule that fills them is
// igemm_plan.h, which only igemm.hip includes.  No HIP.
#pragma once

namespace ldmseg {

enum DType : int { DT_F32 = 0, DT_BF16 = 1 };
enum Epilogue : int {
  EPI_STORE = 0,   // out[m][n] = acc + bias (+rowbias) (+resid), optional SiLU
  EPI_GEGLU = 1,   // packed (a,g) 16-column interleave -> out[m][n/2] = a*gelu(g)
  EPI_NCHW_F32 = 2,  // out is float NCHW [B][n_valid][Ho*Wo]  (conv_out, VAE heads)
  EPI_CONVT2 = 3,  // ConvTranspose2d k2s2: n = tap*Cout + co scattered to (2y+dy,2x+dx)
  EPI_ROWS_F32 = 4,  // out is float row-major [M][ldo] whatever the compute dtype (attention scores of the image VAE)
};

// template instantiation + plan of a launch.  cf: the K slices are finished inside the launch (cf_poll: bound of its partner
// poll in 100 MHz ticks); x3: IgemmParams::x3 (1 = split-bf16 in the K loop, 2 = W holds hi | lo planes)
struct IgemmDispatch { int dtype, bm, bn, wm, wn, nst, pipe, ldr, splits, grid, lnf, cm, cf, xt, up4, x3, cf_poll; };

// What the rule reads of an IgemmParams (all ints, in the order ldmseg_op_igemm_plan takes them).  lnf: a LayerNorm is folded
// (rowstats); region: the caller gave a counter region for the in-launch finish (cf_ctr).
struct IgemmLaunchDesc { int M, N, C0, C1, C2, C3, taps, stride, up, up4, cm, epi, lnf, x3, splits, no_finish, region; };

}  // namespace ldmseg
