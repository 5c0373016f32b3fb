// The scheduler step of a guided sampling loop (classifier-free guidance, trainers_ldm_cond.py:1141-1150).
//
// The UNet ran on 2B images (uncond half first); for every element of the B-image latents:
//   noise_pred = uncond + g * (cond - uncond)      three fp32 ops, each rounded on its own (torch's order)
//   latents    = DDIM step (sched_math.h; the last step keeps pred_original_sample)
// and the updated latents are also written to both halves of the next forward's 2B-image input.  multiplier 1: eps is the
// model output itself.  Built with -ffp-contract=off like sched.hip: the result is bit-identical to the Python loop.
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"
#include "sched_math.h"

namespace ldmseg {
namespace {

__global__ void guided_step_kernel(const float* __restrict__ eps, float* latents, float* cond, float* lat2, size_t n, int mult,
                                   float g, DdimCoef c, int last) {
#pragma clang fp contract(off)
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float e = eps[i];
  if (mult == 2) {
    const float u = e, t = eps[n + i];
    e = __fadd_rn(u, __fmul_rn(g, __fsub_rn(t, u)));
  }
  float prev, x0;
  ddim_update(e, latents[i], c, prev, x0);
  const float nx = last ? x0 : prev;
  latents[i] = nx;
  if (cond) cond[i] = x0;
  if (lat2) { lat2[i] = nx; lat2[n + i] = nx; }
}

}  // namespace

int launch_guided_step(const float* eps, float* latents, float* cond, float* lat2, size_t n, int mult, float g, DdimCoef c,
                       int last, hipStream_t s) {
  if (mult != 1 && mult != 2) return -2;
  LDMSEG_LAUNCH(launch_name("guided_step_kernel"), guided_step_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, eps,
                latents, cond, lat2, n, mult, g, c, last);
  return launch_status();
}

}  // namespace ldmseg
