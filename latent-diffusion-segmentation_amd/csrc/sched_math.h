// The DDIM update of one element (ddim_scheduler.py:238-267), shared by ddim_step_kernel (sched.hip) and the fused step
// tail (tail.hip).  Every product / sum / quotient is rounded separately (__f*_rn; both files are built with
// -ffp-contract=off) so that the result is bit-identical to the reference's chain of torch elementwise ops.
#pragma once
#include "kernels.h"

namespace ldmseg {

__device__ __forceinline__ void ddim_update(float mo, float x, const DdimCoef& c, float& prev, float& x0_out) {
#pragma clang fp contract(off)
  float x0, pe;
  if (c.pred_type == 0) {          // epsilon
    x0 = __fdiv_rn(__fsub_rn(x, __fmul_rn(c.sqrt_b_t, mo)), c.sqrt_a_t);
    pe = mo;
  } else if (c.pred_type == 1) {   // sample
    x0 = mo;
    pe = __fdiv_rn(__fsub_rn(x, __fmul_rn(c.sqrt_a_t, x0)), c.sqrt_b_t);
  } else {                         // v_prediction
    x0 = __fsub_rn(__fmul_rn(c.sqrt_a_t, x), __fmul_rn(c.sqrt_b_t, mo));
    pe = __fadd_rn(__fmul_rn(c.sqrt_a_t, mo), __fmul_rn(c.sqrt_b_t, x));
  }
  if (c.clip) x0 = fminf(fmaxf(x0, -c.clip_range), c.clip_range);
  if (c.use_clipped) pe = __fdiv_rn(__fsub_rn(x, __fmul_rn(c.sqrt_a_t, x0)), c.sqrt_b_t);
  const float dir = __fmul_rn(c.sqrt_b_prev, pe);
  prev = __fadd_rn(__fmul_rn(c.sqrt_a_prev, x0), dir);
  x0_out = x0;
}

// add_noise / remove_noise of one element (ddim_scheduler.py:155-216), shared by add_noise_kernel (sched.hip) and the loss
// tail (loss.hip).  `a` is alphas_cumprod[t]; the two coefficients are formed once per sample, the element op per element.
struct NoiseCoef {
  float sa_scaled;   // sqrt(a) * scale
  float sb;          // sqrt(1 - a)
};

__device__ __forceinline__ int64_t clamp_timestep(int64_t t, int n_train) {
  return t < 0 ? 0 : (t >= n_train ? (int64_t)n_train - 1 : t);
}

__device__ __forceinline__ NoiseCoef noise_coef(float a, float scale) {
#pragma clang fp contract(off)
  NoiseCoef c;
  c.sa_scaled = __fmul_rn(__fsqrt_rn(a), scale);
  c.sb = __fsqrt_rn(__fsub_rn(1.0f, a));
  return c;
}

__device__ __forceinline__ float add_noise_elem(float x0, float noise, const NoiseCoef& c) {
#pragma clang fp contract(off)
  return __fadd_rn(__fmul_rn(c.sa_scaled, x0), __fmul_rn(c.sb, noise));
}

__device__ __forceinline__ float remove_noise_elem(float noisy, float noise, const NoiseCoef& c) {
#pragma clang fp contract(off)
  return __fdiv_rn(__fsub_rn(noisy, __fmul_rn(c.sb, noise)), c.sa_scaled);
}

}  // namespace ldmseg
