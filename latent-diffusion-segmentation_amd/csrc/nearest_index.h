// Source pixel of F.interpolate(mode='nearest') for one output index (the legacy 'nearest', not 'nearest-exact'):
//   scale = float(in_size) / float(out_size)            one fp32 division
//   src   = min(int(floor(float(dst) * scale)), in_size - 1)
// in fp32 like torch's own index computation, so that sizes whose ratio is not exactly representable pick the same pixel.
// Pure: no state, usable on host and device; tests/test_diffusion_loss_cpu.py checks it against torch through
// ldmseg_op_nearest_index for every input size 1..130.
#pragma once

namespace ldmseg {

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LDMSEG_HD __host__ __device__
#else
#define LDMSEG_HD
#endif

LDMSEG_HD constexpr inline float nearest_scale(int in_size, int out_size) { return (float)in_size / (float)out_size; }

LDMSEG_HD constexpr inline int nearest_src_index_scaled(int dst, float scale, int in_size) {
  // dst * scale >= 0: the truncating conversion is the floor
  const int src = (int)((float)dst * scale);
  return src < in_size - 1 ? src : in_size - 1;
}

LDMSEG_HD constexpr inline int nearest_src_index(int dst, int in_size, int out_size) {
  return nearest_src_index_scaled(dst, nearest_scale(in_size, out_size), in_size);
}

#undef LDMSEG_HD

}  // namespace ldmseg
