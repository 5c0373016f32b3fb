// Backward kernels of the seg-VAE decoder: the conv / transposed-conv weight gradient, the LayerNorm2d + SiLU and
// GroupNorm + SiLU backwards, the bias column sums and the weight packings of the data gradients (which run on igemm).
// fp32 tensors throughout.  Every sum over pixels or rows is cut into runs whose partial sums are stored and then added in run
// order by one thread per output: no float atomics, the results are bitwise repeatable.
#include <algorithm>

#include "common.h"
#include "vae_bwd.h"

namespace ldmseg {

namespace {

// ------------------------------------------------------------------ weight gradient
struct WgradArgs {
  const float* dy; const float* x; float* partial;
  int ldy, P, H, W, N, C, taps;
  int n_tiles, c_tiles, tiles, steps, steps_per_slice, items;
  FastDiv fd_hw, fd_w;
};

// A workgroup of four waves owns a 128 (n) x 128 (c) output tile of one tap over one slice of the pixel axis; a wave owns 64 x 64
// of it as 4 x 4 MFMA tiles.  The tap's shift is applied to the pixel of the X operand; a pixel whose neighbour lies outside ITS image
// contributes zero (never the next row's or the next image's pixel).  Rows past P and columns past N / C read nothing and count as zero.
//
// The fp32 form: the contraction index is the pixel and both operands are stored pixel-major, so lane (lg, lr) of a 16-channel
// fragment reads element [pixel(lg)][channel lr] straight from global memory and that value IS its operand of
// v_mfma_f32_16x16x4_f32 (k = lg; eight MFMAs walk the 32 pixels of a step): no transpose, no LDS.
__global__ __launch_bounds__(256) void wgrad_f32_kernel(const WgradArgs p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int HW = p.H * p.W;
  const int KK = p.taps * p.C;
  for (int item = blockIdx.x; item < p.items; item += gridDim.x) {
    const int slice = item / p.tiles, tile = item - slice * p.tiles;
    const int per_tap = p.n_tiles * p.c_tiles;
    const int tap = tile / per_tap, rem_t = tile - tap * per_tap;
    const int nt = rem_t / p.c_tiles, ct = rem_t - nt * p.c_tiles;
    const int n0 = nt * kWgradTileN + (wave >> 1) * 64, c0 = ct * kWgradTileC + (wave & 1) * 64;
    const int dy_ = p.taps == 9 ? tap / 3 - 1 : 0, dx_ = p.taps == 9 ? tap % 3 - 1 : 0;
    const long long shift = (long long)dy_ * p.W + dx_;
    bool nv[4], cv[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) { nv[f] = n0 + 16 * f + lr < p.N; cv[f] = c0 + 16 * f + lr < p.C; }
    f32x4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int s0 = slice * p.steps_per_slice, s1 = min(p.steps, s0 + p.steps_per_slice);
    for (int st = s0; st < s1; ++st) {
      const int pbase = st * kWgradStep;
      float av[4][8], bv[4][8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int pix = pbase + 4 * j + lg;
        const bool pv = pix < p.P;
        bool xv = pv;
        if (p.taps == 9) {
          const int img = fd_div(pix, p.fd_hw);
          const int r = pix - img * HW;
          const int y = fd_div(r, p.fd_w);
          const int xx = r - y * p.W;
          xv = pv && (unsigned)(y + dy_) < (unsigned)p.H && (unsigned)(xx + dx_) < (unsigned)p.W;
        }
        const float* ar = p.dy + (long long)pix * p.ldy + n0 + lr;
        const float* br = p.x + ((long long)pix + shift) * p.C + c0 + lr;
#pragma unroll
        for (int f = 0; f < 4; ++f) {
          av[f][j] = (pv && nv[f]) ? ar[16 * f] : 0.f;
          bv[f][j] = (xv && cv[f]) ? br[16 * f] : 0.f;
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a][j], bv[b][j], acc[a][b], 0, 0, 0);
    }
    // acc[a][b][j] = tile element (row n0 + 16 a + 4 lg + j, column c0 + 16 b + lr)
    float* slab = p.partial + (size_t)slice * p.N * KK + (size_t)tap * p.C;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int c = c0 + 16 * b + lr;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int n = n0 + 16 * a + 4 * lg + j;
          if (n < p.N && c < p.C) slab[(size_t)n * KK + c] = acc[a][b][j];
        }
      }
  }
}

// The split-bf16 form (hi = bf16(x), lo = bf16(x - hi), products lo.hi + hi.lo + hi.hi as igemm's), the split made ONCE per workgroup: the 256 threads load the 32-pixel x 128-channel tiles of both operands
// with 16-byte loads (the next step's loads are in flight under this step's MFMAs), split every value into hi = bf16(x) and
// lo = bf16(x - hi) and store four bf16 planes [pixel][channel] in LDS; the waves then take their operands with the transposed LDS
// read (ds_read_b64_tr_b16: a 16-lane group reads 4 pixel rows x 16 channels and lane i receives channel i of the 4 rows), which
// makes the pixel axis the lane's contiguous K axis.  Lane group lg takes pixel rows 4 lg .. 4 lg + 3 and 16 + 4 lg .. 16 + 4 lg + 3
// of the step as its k = 8 lg .. 8 lg + 7 - any K permutation is legal as long as both operands use the same one - so the two groups
// of a 32-lane half read 8 consecutive rows; rows are 288 bytes apart (128 bf16 + 32 B: 8 banks further per row), which spreads the
// 32 lanes' 8-byte reads over all 64 banks.
constexpr int kWgRow = 288, kWgPlane = 32 * kWgRow;

__device__ __forceinline__ void split4(const float4& v, uint2& hi, uint2& lo) {
  hi.x = pack_bf16x2(v.x, v.y);
  hi.y = pack_bf16x2(v.z, v.w);
  lo.x = pack_bf16x2(v.x - bits_f32(hi.x << 16), v.y - bits_f32(hi.x & 0xffff0000u));
  lo.y = pack_bf16x2(v.z - bits_f32(hi.y << 16), v.w - bits_f32(hi.y & 0xffff0000u));
}

__global__ __launch_bounds__(256) void wgrad_x3_kernel(const WgradArgs p) {
  __shared__ __attribute__((aligned(16))) char lds[4 * kWgPlane];      // A hi | A lo | B hi | B lo
  typedef short s16x4 __attribute__((ext_vector_type(4)));
  typedef __attribute__((address_space(3))) s16x4* lds_v4;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int HW = p.H * p.W;
  const int KK = p.taps * p.C;
  // transposed read: lane 4 q + pp of a group supplies row q, channels 4 pp .. 4 pp + 3 of the block
  const int tr_off = (4 * lg + (lr >> 2)) * kWgRow + (lr & 3) * 8;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int item = blockIdx.x; item < p.items; item += gridDim.x) {
    const int slice = item / p.tiles, tile = item - slice * p.tiles;
    const int per_tap = p.n_tiles * p.c_tiles;
    const int tap = tile / per_tap, rem_t = tile - tap * per_tap;
    const int nt = rem_t / p.c_tiles, ct = rem_t - nt * p.c_tiles;
    const int n0b = nt * kWgradTileN, c0b = ct * kWgradTileC;
    const int wn = (wave >> 1) * 64, wc = (wave & 1) * 64;
    const int dy_ = p.taps == 9 ? tap / 3 - 1 : 0, dx_ = p.taps == 9 ? tap % 3 - 1 : 0;
    const long long shift = (long long)dy_ * p.W + dx_;
    f32x4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int s0 = slice * p.steps_per_slice, s1 = min(p.steps, s0 + p.steps_per_slice);
    float4 ra[4], rb[4];
    // thread t loads float4 (row, c4) = ((t + 256 i) / 32, (t + 256 i) % 32) of both tiles: rows t / 32 + 8 i, one column group
    const int c4 = t & 31, row0 = t >> 5;
    const bool a_ok = n0b + 4 * c4 < p.N, b_ok = c0b + 4 * c4 < p.C;
    auto load = [&](int st) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int pix = st * kWgradStep + row0 + 8 * i;
        const bool pv = pix < p.P;
        bool xv = pv;
        if (p.taps == 9) {
          const int img = fd_div(pix, p.fd_hw);
          const int r = pix - img * HW;
          const int y = fd_div(r, p.fd_w);
          const int xx = r - y * p.W;
          xv = pv && (unsigned)(y + dy_) < (unsigned)p.H && (unsigned)(xx + dx_) < (unsigned)p.W;
        }
        ra[i] = (pv && a_ok) ? *(const float4*)(p.dy + (long long)pix * p.ldy + n0b + 4 * c4) : zero4;
        rb[i] = (xv && b_ok) ? *(const float4*)(p.x + ((long long)pix + shift) * p.C + c0b + 4 * c4) : zero4;
      }
    };
    load(s0);
    for (int st = s0; st < s1; ++st) {
      __syncthreads();                                   // the previous step's reads are done
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int off = (row0 + 8 * i) * kWgRow + c4 * 8;
        uint2 hi, lo;
        split4(ra[i], hi, lo);
        *(uint2*)(lds + off) = hi;
        *(uint2*)(lds + kWgPlane + off) = lo;
        split4(rb[i], hi, lo);
        *(uint2*)(lds + 2 * kWgPlane + off) = hi;
        *(uint2*)(lds + 3 * kWgPlane + off) = lo;
      }
      __syncthreads();
      if (st + 1 < s1) load(st + 1);                     // in flight under the MFMAs below
      bf16x8 ah[4], al[4], bh[4], bl[4];
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        auto frag = [&](int plane, int col) {
          const char* base = lds + plane * kWgPlane + tr_off + col * 2;
          const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(base));
          const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(base + 16 * kWgRow));
          const uint2 u0 = __builtin_bit_cast(uint2, v0), u1 = __builtin_bit_cast(uint2, v1);
          return __builtin_bit_cast(bf16x8, make_uint4(u0.x, u0.y, u1.x, u1.y));
        };
        ah[f] = frag(0, wn + 16 * f); al[f] = frag(1, wn + 16 * f);
        bh[f] = frag(2, wc + 16 * f); bl[f] = frag(3, wc + 16 * f);
      }
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[a], bh[b], acc[a][b], 0, 0, 0);
          acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[a], bl[b], acc[a][b], 0, 0, 0);
          acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[a], bh[b], acc[a][b], 0, 0, 0);
        }
    }
    __syncthreads();                                     // (the next item writes the planes again)
    float* slab = p.partial + (size_t)slice * p.N * KK + (size_t)tap * p.C;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int c = c0b + wc + 16 * b + lr;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int n = n0b + wn + 16 * a + 4 * lg + j;
          if (n < p.N && c < p.C) slab[(size_t)n * KK + c] = acc[a][b][j];
        }
      }
  }
}

// one thread per gradient element: the slabs in slice order
__global__ void wgrad_finish_kernel(const float* __restrict__ partial, int slices, int N, int C, int taps, int form, int n_real, int c_real,
                                    int co, float* __restrict__ out) {
  const int total = n_real * taps * c_real;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int c = idx % c_real, tap = (idx / c_real) % taps, n = idx / (c_real * taps);
  const size_t KK = (size_t)taps * C;
  const float* src = partial + (size_t)n * KK + (size_t)tap * C + c;
  float sum = 0.f;
  for (int s = 0; s < slices; ++s) sum += src[(size_t)s * N * KK];
  if (form == 0) out[((size_t)n * c_real + c) * taps + tap] = sum;
  else out[((size_t)c * co + n % co) * 4 + n / co] = sum;
}

// ------------------------------------------------------------------ column sums (bias gradients) and the slab sum every reduction ends in
constexpr int kColsumRows = 256, kColsumMaxSlices = 1024;

__global__ void colsum_partial_kernel(const float* __restrict__ a, int lda, int P, int N, int rows_per, float* __restrict__ partial) {
  const int col = blockIdx.y * blockDim.x + threadIdx.x;
  if (col >= N) return;
  const int r0 = blockIdx.x * rows_per, r1 = min(P, r0 + rows_per);
  float sum = 0.f;
  for (int r = r0; r < r1; ++r) sum += a[(size_t)r * lda + col];
  partial[(size_t)blockIdx.x * N + col] = sum;
}
// out[j] = sum_{s < S} sum_{q < Q} part[s * stride + q * qstride + j], in that order
__global__ void slab_sum_kernel(const float* __restrict__ part, int S, int stride, int Q, int qstride, int n, float* __restrict__ out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  float sum = 0.f;
  for (int s = 0; s < S; ++s)
    for (int q = 0; q < Q; ++q) sum += part[(size_t)s * stride + (size_t)q * qstride + j];
  out[j] = sum;
}

__device__ __forceinline__ float silu_grad(float u) {
  const float sg = 1.0f / (1.0f + __expf(-u));
  return sg * (1.0f + u * (1.0f - sg));
}

// ------------------------------------------------------------------ LayerNorm2d + SiLU backward
constexpr int kLnBwdPer = 16;          // channels per lane: C <= 1024
constexpr int kLnBwdMaxBlocks = 1024;

// A wave per row; the four waves of a workgroup walk rows [r0, r1) of their run (wave w: r0 + w, r0 + w + 4, ...), every lane adding
// its channels' s * xhat and s in row order; the waves' sums are added in wave order -> partial[run][2][C].
__global__ __launch_bounds__(256) void ln_silu_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          float* __restrict__ dx, float* __restrict__ partial, int M, int C, float eps,
                                                          int rows_per, int pm, int H2, int W2) {
  extern __shared__ float red[];       // [4][2][C]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int per = C >> 6;
  float g[kLnBwdPer], bt[kLnBwdPer], ag[kLnBwdPer], ab[kLnBwdPer];
#pragma unroll
  for (int i = 0; i < kLnBwdPer; ++i) {
    ag[i] = 0.f; ab[i] = 0.f;
    g[i] = i < per ? gamma[lane + 64 * i] : 0.f;
    bt[i] = i < per ? beta[lane + 64 * i] : 0.f;
  }
  const int r0 = blockIdx.x * rows_per, r1 = min(M, r0 + rows_per);
  const float inv_c = 1.0f / (float)C;
  for (int r = r0 + wave; r < r1; r += 4) {
    const float* xr = x + (size_t)r * C;
    const float* dr = dy + (size_t)r * C;
    float xv[kLnBwdPer], gh[kLnBwdPer];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < kLnBwdPer; ++i) { xv[i] = i < per ? xr[lane + 64 * i] : 0.f; sum += xv[i]; }
    const float mean = wave64_sum(sum) * inv_c;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < kLnBwdPer; ++i) if (i < per) { const float d = xv[i] - mean; sq += d * d; }
    const float rstd = rsqrtf(wave64_sum(sq) * inv_c + eps);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < kLnBwdPer; ++i) if (i < per) {
      const float xh = (xv[i] - mean) * rstd;
      const float u = g[i] * xh + bt[i];
      const float sv = dr[lane + 64 * i] * silu_grad(u);
      ag[i] += sv * xh; ab[i] += sv;
      gh[i] = g[i] * sv; xv[i] = xh;
      s1 += gh[i]; s2 += gh[i] * xh;
    }
    const float m1 = wave64_sum(s1) * inv_c, m2 = wave64_sum(s2) * inv_c;
    size_t ro = (size_t)r;
    if (pm) {
      const int hw = H2 * W2;
      const int img = r / hw, rem = r - img * hw;
      const int Y = rem / W2, X = rem - Y * W2;
      ro = (((size_t)img * (H2 >> 1) + (Y >> 1)) * (W2 >> 1) + (X >> 1)) * 4 + 2 * (Y & 1) + (X & 1);
    }
    float* o = dx + ro * C;
#pragma unroll
    for (int i = 0; i < kLnBwdPer; ++i) if (i < per) o[lane + 64 * i] = rstd * (gh[i] - m1 - xv[i] * m2);
  }
  if (!partial) return;
#pragma unroll
  for (int i = 0; i < kLnBwdPer; ++i) if (i < per) {
    red[(wave * 2 + 0) * C + lane + 64 * i] = ag[i];
    red[(wave * 2 + 1) * C + lane + 64 * i] = ab[i];
  }
  __syncthreads();
  for (int j = threadIdx.x; j < 2 * C; j += 256)
    partial[(size_t)blockIdx.x * 2 * C + j] = ((red[j] + red[2 * C + j]) + red[4 * C + j]) + red[6 * C + j];
}

// ------------------------------------------------------------------ GroupNorm + SiLU backward
constexpr int kGnBwdThreads = 512;

// One workgroup per (group, image).  Pass 1: mean and variance of the group (fp64 sums, fixed tree).  Pass 2: thread (ps, j) walks
// pixels ps, ps + PS, ... of channel j of the group and adds s * xhat and s; the PS sums of a channel are added in ps order ->
// pc[image][0 | 1][c]; the group's mean(ghat) and mean(ghat * xhat) follow from them -> gstat[image][group] = {mean, rstd, m1, m2}.
__global__ __launch_bounds__(kGnBwdThreads) void gn_silu_bwd_stats_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                           int HW, int C, int cpg, float eps, float* __restrict__ pc,
                                                                           float* __restrict__ gstat) {
  __shared__ double rd[2 * kGnBwdThreads];
  __shared__ float rf[2 * kGnBwdThreads];
  __shared__ float st[2];
  const int t = threadIdx.x, grp = blockIdx.x, img = blockIdx.y;
  const int PS = kGnBwdThreads / cpg;
  const bool active = t < PS * cpg;
  const int j = t % cpg, ps = t / cpg;
  const int c = grp * cpg + j;
  const float* xb = x + (size_t)img * HW * C + c;
  const float* db = dy + (size_t)img * HW * C + c;
  double sum = 0.0, sq = 0.0;
  if (active)
    for (int pix = ps; pix < HW; pix += PS) { const double v = (double)xb[(size_t)pix * C]; sum += v; sq += v * v; }
  rd[t] = sum; rd[kGnBwdThreads + t] = sq;
  __syncthreads();
  for (int w = kGnBwdThreads / 2; w > 0; w >>= 1) {
    if (t < w) { rd[t] += rd[t + w]; rd[kGnBwdThreads + t] += rd[kGnBwdThreads + t + w]; }
    __syncthreads();
  }
  if (t == 0) {
    const double n = (double)HW * cpg;
    const double m = rd[0] / n;
    double var = rd[kGnBwdThreads] / n - m * m;
    if (var < 0.0) var = 0.0;
    st[0] = (float)m;
    st[1] = (float)(1.0 / sqrt(var + (double)eps));
  }
  __syncthreads();
  const float mean = st[0], rstd = st[1];
  float ag = 0.f, ab = 0.f;
  if (active) {
    const float gm = gamma[c], bt = beta[c];
    for (int pix = ps; pix < HW; pix += PS) {
      const float xh = (xb[(size_t)pix * C] - mean) * rstd;
      const float sv = db[(size_t)pix * C] * silu_grad(gm * xh + bt);
      ag += sv * xh; ab += sv;
    }
  }
  rf[2 * t] = ag; rf[2 * t + 1] = ab;
  __syncthreads();
  if (t < cpg) {
    float sg = 0.f, sb = 0.f;
    for (int q = 0; q < PS; ++q) { sg += rf[2 * (q * cpg + t)]; sb += rf[2 * (q * cpg + t) + 1]; }
    pc[((size_t)img * 2 + 0) * C + c] = sg;
    pc[((size_t)img * 2 + 1) * C + c] = sb;
    rf[2 * t] = gamma[c] * sg; rf[2 * t + 1] = gamma[c] * sb;      // (only threads t < cpg touch these slots now)
  }
  __syncthreads();
  if (t == 0) {
    float m2 = 0.f, m1 = 0.f;
    for (int q = 0; q < cpg; ++q) { m2 += rf[2 * q]; m1 += rf[2 * q + 1]; }
    const float inv_n = 1.0f / ((float)HW * (float)cpg);
    float* o = gstat + ((size_t)img * gridDim.x + grp) * 4;
    o[0] = mean; o[1] = rstd; o[2] = m1 * inv_n; o[3] = m2 * inv_n;
  }
}

__global__ void gn_silu_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ gamma,
                                         const float* __restrict__ beta, const float* __restrict__ gstat, float* __restrict__ dx, int HW,
                                         int C, int cpg, int groups, size_t total) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(e % C);
    const size_t row = e / C;
    const int img = (int)(row / HW);
    const float* gs = gstat + ((size_t)img * groups + c / cpg) * 4;
    const float xh = (x[e] - gs[0]) * gs[1];
    const float gm = gamma[c];
    const float gh = gm * dy[e] * silu_grad(gm * xh + beta[c]);
    dx[e] = gs[1] * (gh - gs[2] - xh * gs[3]);
  }
}

// ------------------------------------------------------------------ weight packings of the data gradients
__global__ void pack_dgrad_conv_kernel(const float* __restrict__ w, float* __restrict__ out, int Co, int Ci, int Npad, int Cop) {
  const size_t total = (size_t)Npad * 9 * Cop;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int co = (int)(i % Cop), t = (int)((i / Cop) % 9), n = (int)(i / ((size_t)9 * Cop));
    out[i] = (n < Ci && co < Co) ? w[((size_t)co * Ci + n) * 9 + (8 - t)] : 0.f;
  }
}
__global__ void pack_dgrad_convt_kernel(const float* __restrict__ w, float* __restrict__ out, int Ci, int Co, int Npad) {
  const size_t K = (size_t)4 * Co, total = (size_t)Npad * K;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int k = (int)(i % K), n = (int)(i / K);
    const int q = k / Co, co = k - q * Co;
    out[i] = n < Ci ? w[((size_t)n * Co + co) * 4 + q] : 0.f;
  }
}

inline int grid_for(size_t n, int cap = 8192) { return (int)std::min<size_t>((size_t)cap, std::max<size_t>(1, (n + 255) / 256)); }

}  // namespace

// ------------------------------------------------------------------ launchers
int wgrad_plan(const WgradParams& p, int cus, WgradPlan* pl) {
  if (p.B < 1 || p.H < 1 || p.W < 1 || (long long)p.B * p.H * p.W >= (1ll << 30)) return -2;
  if (p.N > p.ldy) return -2;
  return wgrad_choose(WgradDesc{p.B * p.H * p.W, p.N, p.C, p.taps, p.x3}, cus, pl);
}
size_t wgrad_partial_bytes(const WgradParams& p, const WgradPlan& pl) {
  return (size_t)pl.slices * p.N * p.taps * p.C * sizeof(float);
}
int launch_wgrad(const WgradParams& p, const WgradPlan& pl, hipStream_t s) {
  if (!p.dy || !p.x || !p.partial) return -2;
  WgradArgs a;
  a.dy = p.dy; a.x = p.x; a.partial = p.partial;
  a.ldy = p.ldy; a.P = p.B * p.H * p.W; a.H = p.H; a.W = p.W; a.N = p.N; a.C = p.C; a.taps = p.taps;
  a.n_tiles = pl.n_tiles; a.c_tiles = pl.c_tiles; a.tiles = pl.tiles; a.steps = pl.steps; a.steps_per_slice = pl.steps_per_slice;
  a.items = pl.items;
  a.fd_hw = fastdiv_make(p.H * p.W); a.fd_w = fastdiv_make(p.W);
  if (pl.x3) LDMSEG_LAUNCH_GEMM(wgrad_plan_name(pl), wgrad_x3_kernel, dim3(pl.grid_x), dim3(pl.block), 0, s, a);
  else LDMSEG_LAUNCH_GEMM(wgrad_plan_name(pl), wgrad_f32_kernel, dim3(pl.grid_x), dim3(pl.block), 0, s, a);
  return launch_status();
}
int launch_wgrad_finish(const WgradParams& p, const WgradPlan& pl, int form, int n_real, int c_real, int co, float* out, hipStream_t s) {
  if (n_real > p.N || c_real > p.C || (form == 1 && (p.taps != 1 || co < 1 || n_real != 4 * co))) return -2;
  const int total = n_real * p.taps * c_real;
  LDMSEG_LAUNCH(form ? "wgrad_finish<convt>" : "wgrad_finish<conv>", wgrad_finish_kernel, dim3((total + 255) / 256), dim3(256), 0, s,
                p.partial, pl.slices, p.N, p.C, p.taps, form, n_real, c_real, co, out);
  return launch_status();
}

int colsum_slices(int P) {
  const int rows = std::max(kColsumRows, (P + kColsumMaxSlices - 1) / kColsumMaxSlices);
  return (P + rows - 1) / rows;
}
size_t colsum_scratch_bytes(int P, int N) { return (size_t)colsum_slices(P) * N * sizeof(float); }
int launch_colsum(const float* a, int lda, int P, int N, int Q, int qstride, int n, float* scratch, float* out, hipStream_t s) {
  if (P < 1 || N < 1 || N > lda || (Q - 1) * qstride + n > N) return -2;
  const int rows = std::max(kColsumRows, (P + kColsumMaxSlices - 1) / kColsumMaxSlices);
  const int S = (P + rows - 1) / rows;
  LDMSEG_LAUNCH("colsum_partial<f32>", colsum_partial_kernel, dim3(S, (N + 127) / 128), dim3(128), 0, s, a, lda, P, N, rows, scratch);
  LDMSEG_LAUNCH("slab_sum<f32>", slab_sum_kernel, dim3((n + 127) / 128), dim3(128), 0, s, scratch, S, N, Q, qstride, n, out);
  return launch_status();
}

static int ln_bwd_rows(int M) { return std::max(64, (M + kLnBwdMaxBlocks - 1) / kLnBwdMaxBlocks); }
size_t ln_bwd_scratch_bytes(int M, int C) {
  const int rows = ln_bwd_rows(M);
  return (size_t)((M + rows - 1) / rows) * 2 * C * sizeof(float);
}
int launch_ln_silu_bwd(const float* x, const float* dy, const float* gamma, const float* beta, float* dx, float* dgamma, float* dbeta,
                       int M, int C, float eps, int pm, int H2, int W2, float* scratch, hipStream_t s) {
  if (M < 1 || C % 64 || C > 64 * kLnBwdPer) return -2;
  if (pm && (H2 < 2 || W2 < 2 || (H2 & 1) || (W2 & 1) || M % (H2 * W2))) return -2;
  const int rows = ln_bwd_rows(M), nb = (M + rows - 1) / rows;
  const bool params = dgamma || dbeta;
  LDMSEG_LAUNCH(pm ? "ln_silu_bwd<f32,pm>" : "ln_silu_bwd<f32>", ln_silu_bwd_kernel, dim3(nb), dim3(256), (size_t)8 * C * sizeof(float), s,
                x, dy, gamma, beta, dx, params ? scratch : (float*)nullptr, M, C, eps, rows, pm, H2, W2);
  if (dgamma) LDMSEG_LAUNCH("slab_sum<f32>", slab_sum_kernel, dim3((C + 127) / 128), dim3(128), 0, s, scratch, nb, 2 * C, 1, 0, C, dgamma);
  if (dbeta) LDMSEG_LAUNCH("slab_sum<f32>", slab_sum_kernel, dim3((C + 127) / 128), dim3(128), 0, s, scratch + C, nb, 2 * C, 1, 0, C, dbeta);
  return launch_status();
}

size_t gn_bwd_scratch_bytes(int B, int C) { return ((size_t)B * 2 * C + (size_t)B * 32 * 4) * sizeof(float); }
int launch_gn_silu_bwd(const float* x, const float* dy, const float* gamma, const float* beta, float* dx, float* dgamma, float* dbeta,
                       int B, int HW, int C, float eps, float* scratch, hipStream_t s) {
  const int groups = 32;
  if (B < 1 || HW < 1 || C % groups || C / groups > kGnBwdThreads) return -2;
  const int cpg = C / groups;
  float* pc = scratch;
  float* gstat = scratch + (size_t)B * 2 * C;
  LDMSEG_LAUNCH("gn_silu_bwd_stats<f32>", gn_silu_bwd_stats_kernel, dim3(groups, B), dim3(kGnBwdThreads), 0, s, x, dy, gamma, beta, HW, C, cpg,
                eps, pc, gstat);
  const size_t total = (size_t)B * HW * C;
  LDMSEG_LAUNCH("gn_silu_bwd_apply<f32>", gn_silu_bwd_apply_kernel, dim3(grid_for(total)), dim3(256), 0, s, x, dy, gamma, beta, gstat, dx, HW, C,
                cpg, groups, total);
  if (dgamma) LDMSEG_LAUNCH("slab_sum<f32>", slab_sum_kernel, dim3((C + 127) / 128), dim3(128), 0, s, pc, B, 2 * C, 1, 0, C, dgamma);
  if (dbeta) LDMSEG_LAUNCH("slab_sum<f32>", slab_sum_kernel, dim3((C + 127) / 128), dim3(128), 0, s, pc + C, B, 2 * C, 1, 0, C, dbeta);
  return launch_status();
}

int launch_pack_dgrad_conv(const float* w, float* out, int Co, int Ci, int Npad, int Cop, hipStream_t s) {
  if (Npad < Ci || Cop < Co) return -2;
  LDMSEG_LAUNCH("pack_dgrad_conv<f32>", pack_dgrad_conv_kernel, dim3(grid_for((size_t)Npad * 9 * Cop)), dim3(256), 0, s, w, out, Co, Ci, Npad, Cop);
  return launch_status();
}
int launch_pack_dgrad_convt(const float* w, float* out, int Ci, int Co, int Npad, hipStream_t s) {
  if (Npad < Ci) return -2;
  LDMSEG_LAUNCH("pack_dgrad_convt<f32>", pack_dgrad_convt_kernel, dim3(grid_for((size_t)Npad * 4 * Co)), dim3(256), 0, s, w, out, Ci, Co, Npad);
  return launch_status();
}

}  // namespace ldmseg
