// Backward kernels of the seg-VAE (decoder: DESIGN 8.6, encoder: 8.7): the conv / transposed-conv weight gradient (stride 1 | 2,
// tiles of 32 | 64 | 128), the LayerNorm2d + SiLU, GroupNorm + SiLU and SiLU backwards, the posterior's backward, the bias column
// sums and the weight packings of the data gradients (which run on igemm).
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
  int ldy, P, H, W, N, C, taps;      // P pixels of the map dY lives on; H x W: the map X lives on
  int Ho, Wo;                        // the map dY lives on (stride 1: H x W)
  int n_tiles, c_tiles, tiles, steps, steps_per_slice, items;
  FastDiv fd_hw, fd_w;               // of Ho * Wo and Wo
};

// A workgroup of four waves owns a 32 FA (n) x 32 FB (c) output tile over one slice of the pixel axis; a wave owns a quarter of it
// as FA x FB MFMA tiles (waves 2 x 2: wave >> 1 picks the rows, wave & 1 the columns).  Four kernels: the per-tap forms own the
// tile of ONE tap (FA, FB in 1 | 2 | 4), the all-taps forms the tile of all nine (FA, FB in 1 | 2); each in fp32 and in split bf16.
// S is the conv's stride (dY lives on the output map).  The pieces they share come first, each stated once.

// pixel `pix` of dY and tap offset (dy_, dx_) -> is the X pixel inside its image, and where (element offset / C).  A pixel whose
// neighbour lies outside ITS image contributes zero (never the next row's or the next image's pixel).
template <int S>
__device__ __forceinline__ bool wgrad_x_pixel(const WgradArgs& p, int pix, int dy_, int dx_, long long shift, long long* xrow) {
  const int HWo = p.Ho * p.Wo;
  const int img = fd_div(pix, p.fd_hw);
  const int r = pix - img * HWo;
  const int y = fd_div(r, p.fd_w);
  const int xx = r - y * p.Wo;
  if (S == 1) {
    *xrow = (long long)pix + shift;
    return (unsigned)(y + dy_) < (unsigned)p.H && (unsigned)(xx + dx_) < (unsigned)p.W;
  }
  const int iy = S * y + dy_, ix = S * xx + dx_;
  *xrow = ((long long)img * p.H + iy) * p.W + ix;
  return (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
}

// the K steps [s0, s1) of a slice
__device__ __forceinline__ void wgrad_steps(const WgradArgs& p, int slice, int* s0, int* s1) {
  *s0 = slice * p.steps_per_slice;
  *s1 = min(p.steps, *s0 + p.steps_per_slice);
}
// work item of a per-tap form -> slice, tap, n tile, c tile, the tap's offset on the map of X (and as a pixel shift), its steps
struct WgradItem { int slice, tap, nt, ct, dy_, dx_, s0, s1; long long shift; };
__device__ __forceinline__ WgradItem wgrad_item(const WgradArgs& p, int item) {
  WgradItem w;
  w.slice = item / p.tiles;
  const int tile = item - w.slice * p.tiles;
  const int per_tap = p.n_tiles * p.c_tiles;
  w.tap = tile / per_tap;
  const int rem_t = tile - w.tap * per_tap;
  w.nt = rem_t / p.c_tiles; w.ct = rem_t - w.nt * p.c_tiles;
  w.dy_ = p.taps == 9 ? w.tap / 3 - 1 : 0; w.dx_ = p.taps == 9 ? w.tap % 3 - 1 : 0;
  w.shift = (long long)w.dy_ * p.W + w.dx_;
  wgrad_steps(p, w.slice, &w.s0, &w.s1);
  return w;
}

template <int FA, int FB>
__device__ __forceinline__ void wgrad_clear(f32x4 (&acc)[FA][FB]) {
#pragma unroll
  for (int a = 0; a < FA; ++a)
#pragma unroll
    for (int b = 0; b < FB; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
}
// acc[a][b][j] = tile element (row row0 + 16 a + j, column col0 + 16 b) for the lane's row0 = n0 + 4 lg, col0 = c0 + lr: stored to
// slab[row][col] (KK floats per row) where row < N and col < C.  Rows past N and columns past C were computed from zeros.
template <int FA, int FB>
__device__ __forceinline__ void wgrad_store(const f32x4 (&acc)[FA][FB], float* slab, int KK, int row0, int col0, int N, int C) {
#pragma unroll
  for (int a = 0; a < FA; ++a)
#pragma unroll
    for (int b = 0; b < FB; ++b) {
      const int c = col0 + 16 * b;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = row0 + 16 * a + j;
        if (n < N && c < C) slab[(size_t)n * KK + c] = acc[a][b][j];
      }
    }
}

// The fp32 forms: the contraction index is the pixel and both operands are stored pixel-major, so lane (lg, lr) of a 16-channel
// fragment reads element [pixel(lg)][channel lr] straight from global memory and that value IS its operand of
// v_mfma_f32_16x16x4_f32 (k = lg; eight MFMAs walk the 32 pixels of a step): no transpose, no LDS.  Rows past P and channels past
// the operand's width read nothing and count as zero: v[f] = does the lane's channel ch0 + 16 f of fragment f exist.
template <int F>
__device__ __forceinline__ void wgrad_valid(bool (&v)[F], int ch0, int width) {
#pragma unroll
  for (int f = 0; f < F; ++f) v[f] = ch0 + 16 * f < width;
}

// The split-bf16 forms (hi = bf16(x), lo = bf16(x - hi), products lo.hi + hi.lo + hi.hi as igemm's), the split made ONCE per
// workgroup: the 256 threads load a 32-pixel x 32 F channel tile of an operand with 16-byte loads, split every value and store two
// bf16 planes [pixel][channel] in LDS; the waves then take their operands with the transposed LDS read (ds_read_b64_tr_b16: a
// 16-lane group reads 4 pixel rows x 16 channels and lane i receives channel i of the 4 rows), which makes the pixel axis the lane's
// contiguous K axis.  Lane group lg takes pixel rows 4 lg .. 4 lg + 3 and 16 + 4 lg .. 16 + 4 lg + 3 of the step as its
// k = 8 lg .. 8 lg + 7 - any K permutation is legal as long as both operands use the same one - so the two groups of a 32-lane half
// read 8 consecutive rows; rows are the tile's bf16 width + 32 B apart (288, 160 or 96 bytes = 72, 40 or 24 banks: an odd multiple
// of 8 in each case, so 8 consecutive rows start on the 8 different multiples of 8 banks), which spreads the 32 lanes' 8-byte reads
// over all 64 banks.
constexpr int wg_row(int F) { return 64 * F + 32; }       // bytes between pixel rows of a plane 32 F channels wide
constexpr int wg_plane(int F) { return 32 * wg_row(F); }  // bytes of a plane
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4* lds_v4;

// thread t holds float4 number t + 256 i (i < F) of a tile of 8 F float4 per pixel row: its pixel row and first channel
struct X3Slot { int row, ch; };
template <int F>
__device__ __forceinline__ X3Slot x3_slot(int t, int i) {
  const int idx = t + 256 * i;
  return {idx / (8 * F), 4 * (idx % (8 * F))};
}
// the 16-byte load of a slot: the caller names the source row (its first element and whether it exists) and the channel bound
__device__ __forceinline__ float4 x3_load(bool ok, const float* base, long long at) {
  return ok ? *(const float4*)(base + at) : make_float4(0.f, 0.f, 0.f, 0.f);
}
__device__ __forceinline__ void split4(const float4& v, uint2& hi, uint2& lo) {
  hi.x = pack_bf16x2(v.x, v.y);
  hi.y = pack_bf16x2(v.z, v.w);
  lo.x = pack_bf16x2(v.x - bits_f32(hi.x << 16), v.y - bits_f32(hi.x & 0xffff0000u));
  lo.y = pack_bf16x2(v.z - bits_f32(hi.y << 16), v.w - bits_f32(hi.y & 0xffff0000u));
}
// the thread's F loaded float4, split and stored into the planes at byte offsets hi and lo of the LDS block
template <int F>
__device__ __forceinline__ void x3_stage(char* lds, int hi, int lo, const float4 (&r)[F], int t) {
#pragma unroll
  for (int i = 0; i < F; ++i) {
    const X3Slot s = x3_slot<F>(t, i);
    const int off = s.row * wg_row(F) + s.ch * 2;
    uint2 h, l;
    split4(r[i], h, l);
    *(uint2*)(lds + hi + off) = h;
    *(uint2*)(lds + lo + off) = l;
  }
}
// transposed read: lane 4 q + pp of a group supplies row q, channels 4 pp .. 4 pp + 3 of the block -> the lane's byte offset
template <int F>
__device__ __forceinline__ int x3_lane_offset(int lg, int lr) { return (4 * lg + (lr >> 2)) * wg_row(F) + (lr & 3) * 8; }
// the lane's k = 8 lg .. 8 lg + 7 of a 16-channel block: two transposed reads 16 pixel rows apart
__device__ __forceinline__ bf16x8 x3_frag(const char* base, int row) {
  const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(base));
  const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(base + 16 * row));
  const uint2 u0 = __builtin_bit_cast(uint2, v0), u1 = __builtin_bit_cast(uint2, v1);
  return __builtin_bit_cast(bf16x8, make_uint4(u0.x, u0.y, u1.x, u1.y));
}
// the wave's F fragments of a hi / lo plane pair; at = the lane's offset + 2 bytes x the wave's first channel
template <int F>
__device__ __forceinline__ void x3_frags(bf16x8 (&h)[F], bf16x8 (&l)[F], const char* lds, int hi, int lo, int at) {
#pragma unroll
  for (int f = 0; f < F; ++f) {
    h[f] = x3_frag(lds + hi + at + 32 * f, wg_row(F));
    l[f] = x3_frag(lds + lo + at + 32 * f, wg_row(F));
  }
}
// c += lo.hi + hi.lo + hi.hi, smallest products first: this order is the bits.  (One accumulator tile per call, the loops over the
// wave's tiles stay in the kernels: taken as a whole FA x FB update next to x3_frags, the 64 x 64 all-taps kernel came out with
// another interleaving of reads, writes and MFMAs and 12 more AGPRs.)
__device__ __forceinline__ void x3_mac(f32x4& c, const bf16x8& ah, const bf16x8& al, const bf16x8& bh, const bf16x8& bl) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, c, 0, 0, 0);
}

// ------------------------------------------------------------------ one tile per tap
// fp32, register-only: per step a lane loads its 8 pixels x (FA + FB) channels, then the 8 FA FB MFMAs run.  The tap's shift is
// applied to the pixel of the X operand.
template <int FA, int FB, int S>
__global__ __launch_bounds__(256) void wgrad_f32_kernel(const WgradArgs p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int KK = p.taps * p.C;
  for (int item = blockIdx.x; item < p.items; item += gridDim.x) {
    const WgradItem w = wgrad_item(p, item);
    const int n0 = w.nt * (32 * FA) + (wave >> 1) * (16 * FA), c0 = w.ct * (32 * FB) + (wave & 1) * (16 * FB);
    bool nv[FA], cv[FB];
    wgrad_valid(nv, n0 + lr, p.N);
    wgrad_valid(cv, c0 + lr, p.C);
    f32x4 acc[FA][FB];
    wgrad_clear(acc);
    for (int st = w.s0; st < w.s1; ++st) {
      const int pbase = st * kWgradStep;
      float av[FA][8], bv[FB][8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int pix = pbase + 4 * j + lg;
        const bool pv = pix < p.P;
        bool xv = pv;
        long long xrow = pix;
        if (p.taps == 9) xv = wgrad_x_pixel<S>(p, pix, w.dy_, w.dx_, w.shift, &xrow) && pv;
        const float* ar = p.dy + (long long)pix * p.ldy + n0 + lr;
        const float* br = p.x + xrow * p.C + c0 + lr;
#pragma unroll
        for (int f = 0; f < FA; ++f) av[f][j] = (pv && nv[f]) ? ar[16 * f] : 0.f;
#pragma unroll
        for (int f = 0; f < FB; ++f) bv[f][j] = (xv && cv[f]) ? br[16 * f] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int a = 0; a < FA; ++a)
#pragma unroll
          for (int b = 0; b < FB; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a][j], bv[b][j], acc[a][b], 0, 0, 0);
    }
    wgrad_store(acc, p.partial + (size_t)w.slice * p.N * KK + (size_t)w.tap * p.C, KK, n0 + 4 * lg, c0 + lr, p.N, p.C);
  }
}

// split bf16: four planes (A hi | A lo | B hi | B lo), two barriers per step; the next step's loads are in flight under this step's
// MFMAs.
template <int FA, int FB, int S>
__global__ __launch_bounds__(256) void wgrad_x3_kernel(const WgradArgs p) {
  constexpr int PA = wg_plane(FA), PB = wg_plane(FB);
  constexpr int A_HI = 0, A_LO = PA, B_HI = 2 * PA, B_LO = 2 * PA + PB;
  __shared__ __attribute__((aligned(16))) char lds[2 * PA + 2 * PB];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int KK = p.taps * p.C;
  const int wn = (wave >> 1) * (16 * FA), wc = (wave & 1) * (16 * FB);
  const int at_a = x3_lane_offset<FA>(lg, lr) + 2 * wn, at_b = x3_lane_offset<FB>(lg, lr) + 2 * wc;
  for (int item = blockIdx.x; item < p.items; item += gridDim.x) {
    const WgradItem w = wgrad_item(p, item);
    const int n0b = w.nt * (32 * FA), c0b = w.ct * (32 * FB);
    f32x4 acc[FA][FB];
    wgrad_clear(acc);
    float4 ra[FA], rb[FB];
    auto load = [&](int st) {
#pragma unroll
      for (int i = 0; i < FA; ++i) {
        const X3Slot sl = x3_slot<FA>(t, i);
        const int pix = st * kWgradStep + sl.row;
        ra[i] = x3_load(pix < p.P && n0b + sl.ch < p.N, p.dy, (long long)pix * p.ldy + n0b + sl.ch);
      }
#pragma unroll
      for (int i = 0; i < FB; ++i) {
        const X3Slot sl = x3_slot<FB>(t, i);
        const int pix = st * kWgradStep + sl.row;
        bool xv = pix < p.P;
        long long xrow = pix;
        if (p.taps == 9) xv = wgrad_x_pixel<S>(p, pix, w.dy_, w.dx_, w.shift, &xrow) && xv;
        rb[i] = x3_load(xv && c0b + sl.ch < p.C, p.x, xrow * p.C + c0b + sl.ch);
      }
    };
    load(w.s0);
    for (int st = w.s0; st < w.s1; ++st) {
      __syncthreads();                                   // the previous step's reads are done
      x3_stage<FA>(lds, A_HI, A_LO, ra, t);
      x3_stage<FB>(lds, B_HI, B_LO, rb, t);
      __syncthreads();
      if (st + 1 < w.s1) load(st + 1);                   // in flight under the MFMAs below
      bf16x8 ah[FA], al[FA], bh[FB], bl[FB];
      x3_frags<FA>(ah, al, lds, A_HI, A_LO, at_a);
      x3_frags<FB>(bh, bl, lds, B_HI, B_LO, at_b);
#pragma unroll
      for (int a = 0; a < FA; ++a)
#pragma unroll
        for (int b = 0; b < FB; ++b) x3_mac(acc[a][b], ah[a], al[a], bh[b], bl[b]);
    }
    __syncthreads();                                     // (the next item writes the planes again)
    wgrad_store(acc, p.partial + (size_t)w.slice * p.N * KK + (size_t)w.tap * p.C, KK, n0b + wn + 4 * lg, c0b + wc + lr, p.N, p.C);
  }
}

// ------------------------------------------------------------------ the all-taps tiles of the narrow 3x3 layers
// A workgroup owns ALL NINE taps of a 32 FA (n) x 32 FB (c) tile (the whole layer) over one slice of the pixel axis: N x 9 C
// outputs, an item is a slice.  dY is read once per step and serves the nine taps; X is read at the nine shifted pixels (its halo),
// lines the same workgroup read a row of the map earlier.  A wave holds 9 x FA x FB accumulator tiles.
// fp32, register-only as wgrad_f32_kernel: per four pixels a lane loads its dY values once and one X value per tap.
template <int FA, int FB, int S>
__global__ __launch_bounds__(256) void wgrad9_f32_kernel(const WgradArgs p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int KK = 9 * p.C;
  const int n0 = (wave >> 1) * (16 * FA), c0 = (wave & 1) * (16 * FB);
  bool nv[FA], cv[FB];
  wgrad_valid(nv, n0 + lr, p.N);
  wgrad_valid(cv, c0 + lr, p.C);
  for (int slice = blockIdx.x; slice < p.items; slice += gridDim.x) {
    f32x4 acc[9][FA][FB];
#pragma unroll
    for (int t = 0; t < 9; ++t) wgrad_clear(acc[t]);
    int s0, s1;
    wgrad_steps(p, slice, &s0, &s1);
    for (int st = s0; st < s1; ++st) {
#pragma unroll 2
      for (int j = 0; j < 8; ++j) {
        const int pix = st * kWgradStep + 4 * j + lg;
        const bool pv = pix < p.P;
        const float* ar = p.dy + (long long)pix * p.ldy + n0 + lr;
        float av[FA];
#pragma unroll
        for (int f = 0; f < FA; ++f) av[f] = (pv && nv[f]) ? ar[16 * f] : 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          const int dy_ = t / 3 - 1, dx_ = t % 3 - 1;
          long long xrow;
          const bool xv = wgrad_x_pixel<S>(p, pix, dy_, dx_, (long long)dy_ * p.W + dx_, &xrow) && pv;
          const float* br = p.x + xrow * p.C + c0 + lr;
          float bv[FB];
#pragma unroll
          for (int f = 0; f < FB; ++f) bv[f] = (xv && cv[f]) ? br[16 * f] : 0.f;
#pragma unroll
          for (int a = 0; a < FA; ++a)
#pragma unroll
            for (int b = 0; b < FB; ++b) acc[t][a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a], bv[b], acc[t][a][b], 0, 0, 0);
        }
      }
    }
    float* slab = p.partial + (size_t)slice * p.N * KK;
#pragma unroll
    for (int t = 0; t < 9; ++t) wgrad_store(acc[t], slab + t * p.C, KK, n0 + 4 * lg, c0 + lr, p.N, p.C);
  }
}

// split bf16: per step the dY tile is loaded, split and stored to LDS ONCE and its fragments stay in registers for the nine taps;
// the X planes are made per tap ROW (three taps: 6 planes of 32 pixels), so a step has three rounds of two barriers instead of
// nine.  The next round's X loads (the next step's dY loads with the last round) are in flight under the MFMAs.  LDS: 2 A planes +
// 6 B planes (A hi | A lo | B hi [3 taps] | B lo [3 taps]), 24 - 40 KB.
template <int FA, int FB, int S>
__global__ __launch_bounds__(256) void wgrad9_x3_kernel(const WgradArgs p) {
  constexpr int PA = wg_plane(FA), PB = wg_plane(FB);
  constexpr int A_HI = 0, A_LO = PA, B_HI = 2 * PA, B_LO = 2 * PA + 3 * PB;
  __shared__ __attribute__((aligned(16))) char lds[2 * PA + 6 * PB];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int KK = 9 * p.C;
  const int wn = (wave >> 1) * (16 * FA), wc = (wave & 1) * (16 * FB);
  const int at_a = x3_lane_offset<FA>(lg, lr) + 2 * wn, at_b = x3_lane_offset<FB>(lg, lr) + 2 * wc;
  for (int slice = blockIdx.x; slice < p.items; slice += gridDim.x) {
    f32x4 acc[9][FA][FB];
#pragma unroll
    for (int q = 0; q < 9; ++q) wgrad_clear(acc[q]);
    int s0, s1;
    wgrad_steps(p, slice, &s0, &s1);
    float4 ra[FA], rb[3][FB];
    auto load_a = [&](int st) {
#pragma unroll
      for (int i = 0; i < FA; ++i) {
        const X3Slot sl = x3_slot<FA>(t, i);
        const int pix = st * kWgradStep + sl.row;
        ra[i] = x3_load(pix < p.P && sl.ch < p.N, p.dy, (long long)pix * p.ldy + sl.ch);
      }
    };
    auto load_b = [&](int st, int g) {                    // tap row g: taps 3 g .. 3 g + 2
#pragma unroll
      for (int i = 0; i < FB; ++i) {
        const X3Slot sl = x3_slot<FB>(t, i);
        const int pix = st * kWgradStep + sl.row;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const int dy_ = g - 1, dx_ = q - 1;
          long long xrow;
          const bool xv = wgrad_x_pixel<S>(p, pix, dy_, dx_, (long long)dy_ * p.W + dx_, &xrow) && pix < p.P;
          rb[q][i] = x3_load(xv && sl.ch < p.C, p.x, xrow * p.C + sl.ch);
        }
      }
    };
    load_a(s0);
    load_b(s0, 0);
    for (int st = s0; st < s1; ++st) {
      bf16x8 ah[FA], al[FA];
#pragma unroll
      for (int g = 0; g < 3; ++g) {
        __syncthreads();                                 // the previous round's reads are done
        if (g == 0) x3_stage<FA>(lds, A_HI, A_LO, ra, t);
#pragma unroll
        for (int q = 0; q < 3; ++q) x3_stage<FB>(lds, B_HI + q * PB, B_LO + q * PB, rb[q], t);
        __syncthreads();
        if (g < 2) load_b(st, g + 1);                    // in flight under the MFMAs below
        else if (st + 1 < s1) { load_a(st + 1); load_b(st + 1, 0); }
        if (g == 0) x3_frags<FA>(ah, al, lds, A_HI, A_LO, at_a);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          bf16x8 bh[FB], bl[FB];
          x3_frags<FB>(bh, bl, lds, B_HI + q * PB, B_LO + q * PB, at_b);
#pragma unroll
          for (int a = 0; a < FA; ++a)
#pragma unroll
            for (int b = 0; b < FB; ++b) x3_mac(acc[3 * g + q][a][b], ah[a], al[a], bh[b], bl[b]);
        }
      }
    }
    __syncthreads();                                     // (the next slice writes the planes again)
    float* slab = p.partial + (size_t)slice * p.N * KK;
#pragma unroll
    for (int q = 0; q < 9; ++q) wgrad_store(acc[q], slab + q * p.C, KK, wn + 4 * lg, wc + lr, p.N, p.C);
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

// ------------------------------------------------------------------ SiLU forward / backward on kept pre-activations, posterior backward
// (du may be da itself: no __restrict__ on the pair)
__global__ void silu_bwd_kernel(const float* __restrict__ u, const float* da, float* du, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) du[i] = da[i] * silu_grad(u[i]);
}
__global__ void silu_fwd_kernel(const float* __restrict__ u, float* __restrict__ a, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) a[i] = silu_f(u[i]);   // igemm's epilogue form
}
// dmom [B][8][HW] from dz [B][4][HW]: one thread per element of dz writes the mean and the logvar gradient of its latent
__global__ void posterior_bwd_kernel(const float* __restrict__ mom, const float* __restrict__ noise, float scale, const float* __restrict__ dz,
                                     float* __restrict__ dmom, int HW, size_t total) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t pix = i % HW, r = i / HW;
    const size_t c = r % 4, b = r / 4;
    const float g = dz[i] * scale;
    const float lv = mom[(b * 8 + 4 + c) * HW + pix];
    dmom[(b * 8 + c) * HW + pix] = g;
    // (a NaN logvar fails both comparisons: zero, as the clamp's mask gives)
    dmom[(b * 8 + 4 + c) * HW + pix] = (noise && lv >= -30.f && lv <= 20.f) ? g * noise[i] * 0.5f * expf(0.5f * lv) : 0.f;
  }
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
    float* o = dx + (pm ? phase_major_row(r, H2, W2) : (size_t)r) * C;
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
__global__ void pack_dgrad_conv_s2_kernel(const float* __restrict__ w, float* __restrict__ out, int Co, int Ci, int Npad, int Cop) {
  const size_t total = (size_t)Npad * 9 * Cop;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int co = (int)(i % Cop), t = (int)((i / Cop) % 9), n = (int)(i / ((size_t)9 * Cop));
    const int q = n / Ci, ci = n - q * Ci;
    const int ky = (q >> 1) + 3 - 2 * (t / 3), kx = (q & 1) + 3 - 2 * (t % 3);
    const bool ok = q < 4 && co < Co && (unsigned)ky < 3u && (unsigned)kx < 3u;
    out[i] = ok ? w[((size_t)co * Ci + ci) * 9 + ky * 3 + kx] : 0.f;
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
  const int P = p.B * conv_out_dim(p.H, p.stride) * conv_out_dim(p.W, p.stride);
  return wgrad_choose(WgradDesc{P, p.N, p.C, p.taps, p.x3, p.stride}, p.rule, cus, pl);
}
static int g_wgrad_cus = 0;          // debug key 26
void wgrad_set_cus(int cus) { g_wgrad_cus = cus < 0 ? 0 : cus; }
int wgrad_get_cus() { return g_wgrad_cus; }
int wgrad_cus() { return g_wgrad_cus > 0 ? g_wgrad_cus : num_cus(); }
size_t wgrad_partial_bytes(const WgradParams& p, const WgradPlan& pl) {
  return (size_t)pl.slices * p.N * p.taps * p.C * sizeof(float);
}

namespace {
// Every weight-gradient kernel the library holds, one row each: (all_taps, x3, tile_n, tile_c, stride) -> kernel, the only place
// that names template arguments.  The rows are what a chooser (wgrad_plan.h) can name: per tap the tile pairs with a 128 in them
// ((128, 128) at stride 1 is also the decoder's rule and every one-tap launch), all taps the pairs within 64.  A per-tap kernel with
// both tiles <= 64 has no caller, so it is not built; bringing one back is one row.
typedef void (*WgradKernel)(const WgradArgs);
struct WgradRow { int all_taps, x3, tile_n, tile_c, stride; WgradKernel kernel; };
#define LDMSEG_WGRAD_ROWS(ALL, F32, X3, TN, TC)                                                         \
  {ALL, 0, TN, TC, 1, F32<TN / 32, TC / 32, 1>}, {ALL, 0, TN, TC, 2, F32<TN / 32, TC / 32, 2>},         \
  {ALL, 1, TN, TC, 1, X3<TN / 32, TC / 32, 1>}, {ALL, 1, TN, TC, 2, X3<TN / 32, TC / 32, 2>}
#define LDMSEG_WGRAD_PER_TAP(TN, TC) LDMSEG_WGRAD_ROWS(0, wgrad_f32_kernel, wgrad_x3_kernel, TN, TC)
#define LDMSEG_WGRAD_ALL_TAPS(TN, TC) LDMSEG_WGRAD_ROWS(1, wgrad9_f32_kernel, wgrad9_x3_kernel, TN, TC)
const WgradRow kWgradKernels[] = {
    LDMSEG_WGRAD_PER_TAP(128, 128), LDMSEG_WGRAD_PER_TAP(128, 64), LDMSEG_WGRAD_PER_TAP(128, 32),
    LDMSEG_WGRAD_PER_TAP(64, 128),  LDMSEG_WGRAD_PER_TAP(32, 128),
    LDMSEG_WGRAD_ALL_TAPS(64, 64),  LDMSEG_WGRAD_ALL_TAPS(64, 32), LDMSEG_WGRAD_ALL_TAPS(32, 64), LDMSEG_WGRAD_ALL_TAPS(32, 32)};
#undef LDMSEG_WGRAD_ALL_TAPS
#undef LDMSEG_WGRAD_PER_TAP
#undef LDMSEG_WGRAD_ROWS
static_assert(sizeof(kWgradKernels) / sizeof(kWgradKernels[0]) == 36, "weight-gradient kernel table");
}  // namespace

int launch_wgrad(const WgradParams& p, const WgradPlan& pl, const WgradOut& o, hipStream_t s) {
  if (!p.dy || !p.x || !p.partial || !o.out || pl.stride != p.stride) return -2;
  if (o.n_real > p.N || o.c_real > p.C || (o.form == 1 && (p.taps != 1 || o.co < 1 || o.n_real != 4 * o.co))) return -2;
  if (pl.all_taps && (p.taps != 9 || pl.n_tiles != 1 || pl.c_tiles != 1 || pl.items != pl.slices)) return -2;
  const WgradRow* row = nullptr;
  for (const WgradRow& r : kWgradKernels)
    if (r.all_taps == pl.all_taps && r.x3 == pl.x3 && r.tile_n == pl.tile_n && r.tile_c == pl.tile_c && r.stride == pl.stride) row = &r;
  if (!row) return -2;
  WgradArgs a;
  a.dy = p.dy; a.x = p.x; a.partial = p.partial;
  a.Ho = conv_out_dim(p.H, p.stride); a.Wo = conv_out_dim(p.W, p.stride);
  a.ldy = p.ldy; a.P = p.B * a.Ho * a.Wo; a.H = p.H; a.W = p.W; a.N = p.N; a.C = p.C; a.taps = p.taps;
  a.n_tiles = pl.n_tiles; a.c_tiles = pl.c_tiles; a.tiles = pl.tiles; a.steps = pl.steps; a.steps_per_slice = pl.steps_per_slice;
  a.items = pl.items;
  a.fd_hw = fastdiv_make(a.Ho * a.Wo); a.fd_w = fastdiv_make(a.Wo);
  LDMSEG_LAUNCH_GEMM(wgrad_plan_name(pl), row->kernel, dim3(pl.grid_x), dim3(pl.block), 0, s, a);
  if (const int e = launch_status()) return e;
  const int total = o.n_real * p.taps * o.c_real;
  LDMSEG_LAUNCH(o.form ? "wgrad_finish<convt>" : "wgrad_finish<conv>", wgrad_finish_kernel, dim3((total + 255) / 256), dim3(256), 0, s,
                p.partial, pl.slices, p.N, p.C, p.taps, o.form, o.n_real, o.c_real, o.co, o.out);
  return launch_status();
}

static int colsum_rows(int P) { return std::max(kColsumRows, (P + kColsumMaxSlices - 1) / kColsumMaxSlices); }   // rows per run
int colsum_slices(int P) { return (P + colsum_rows(P) - 1) / colsum_rows(P); }
size_t colsum_scratch_bytes(int P, int N) { return (size_t)colsum_slices(P) * N * sizeof(float); }
int launch_colsum(const float* a, int lda, int P, int N, int Q, int qstride, int n, float* scratch, float* out, hipStream_t s) {
  if (P < 1 || N < 1 || N > lda || (Q - 1) * qstride + n > N) return -2;
  const int rows = colsum_rows(P), S = colsum_slices(P);
  LDMSEG_LAUNCH("colsum_partial<f32>", colsum_partial_kernel, dim3(S, (N + 127) / 128), dim3(128), 0, s, a, lda, P, N, rows, scratch);
  LDMSEG_LAUNCH("slab_sum<f32>", slab_sum_kernel, dim3((n + 127) / 128), dim3(128), 0, s, scratch, S, N, Q, qstride, n, out);
  return launch_status();
}

int launch_silu_bwd(const float* u, const float* da, float* du, size_t n, hipStream_t s) {
  if (!u || !da || !du || n < 1) return -2;
  LDMSEG_LAUNCH("silu_bwd<f32>", silu_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, s, u, da, du, n);
  return launch_status();
}
int launch_silu_fwd(const float* u, float* a, size_t n, hipStream_t s) {
  if (!u || !a || n < 1) return -2;
  LDMSEG_LAUNCH("silu_fwd<f32>", silu_fwd_kernel, dim3(grid_for(n)), dim3(256), 0, s, u, a, n);
  return launch_status();
}
int launch_posterior_backward(const float* moments, const float* noise, float scale, const float* dz, float* dmoments, int B, int HW,
                              hipStream_t s) {
  if (!moments || !dz || !dmoments || B < 1 || HW < 1) return -2;
  const size_t total = (size_t)B * 4 * HW;
  LDMSEG_LAUNCH("posterior_bwd<f32>", posterior_bwd_kernel, dim3(grid_for(total)), dim3(256), 0, s, moments, noise, scale, dz, dmoments, HW, total);
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
int launch_pack_dgrad_conv_s2(const float* w, float* out, int Co, int Ci, int Npad, int Cop, hipStream_t s) {
  if (Npad < 4 * Ci || Cop < Co) return -2;
  LDMSEG_LAUNCH("pack_dgrad_conv_s2<f32>", pack_dgrad_conv_s2_kernel, dim3(grid_for((size_t)Npad * 9 * Cop)), dim3(256), 0, s, w, out, Co, Ci, Npad, Cop);
  return launch_status();
}
int launch_pack_dgrad_convt(const float* w, float* out, int Ci, int Co, int Npad, hipStream_t s) {
  if (Npad < Ci) return -2;
  LDMSEG_LAUNCH("pack_dgrad_convt<f32>", pack_dgrad_convt_kernel, dim3(grid_for((size_t)Npad * 4 * Co)), dim3(256), 0, s, w, out, Ci, Co, Npad);
  return launch_status();
}

}  // namespace ldmseg
