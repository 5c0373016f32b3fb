// Device-side panoptic-quality meter: what pq_compute_annotations (evaluations/panoptic_evaluation_agnostic.py, the restated
// panopticapi rule) does for one (ground truth, prediction) pair, for a whole batch, without a pixel map leaving the GPU.
//
//   pass A (contingency): per pixel the ground-truth id is mapped to a row
//              row 0        VOID (id 0)
//              rows 1..G    the image's declared segments ("slots", ascending id), found by binary search in LDS
//              row G + 1    painted but not declared: neither void nor matchable, still part of the prediction's area
//            and inter[row][pred] += 1, an int32 table [G + 2][P + 1] of the image inside the batch's [B][Gpad + 2][P + 1].
//            A workgroup walks a contiguous chunk of pixels.  Panoptic maps are long runs of one (row, pred) pair: lanes of a
//            wave that hold the same pair as their left neighbour are merged into the run's first lane, which adds the run
//            length.  When the image's (G + 2) * (P + 1) table fits the LDS budget it is privatised per workgroup and only its
//            non-zero cells are added to global memory; otherwise the run heads add straight to global memory.
//   pass B (matching): one workgroup per image: area_pred = column sums, area_gt = given area or row sum, IoU > 0.5 matching
//            with the union reduced by the prediction's overlap with VOID, crowd / void forgiveness of unmatched predictions.
//
// Every counter is an integer added with integer atomics (the same in any order); every division is one IEEE double division
// of two exactly converted integers, i.e. bit-identical to Python's int / int.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/ldmseg_hip.h"
#include "common.h"

namespace ldmseg {
namespace {

constexpr int kPqThreads = 256;
constexpr int kPqChunk = 4096;                 // pixels per workgroup in pass A (16 rounds of 256)
constexpr int kPqLdsBytes = 64 * 1024;         // privatise when ids + table fit: at least two workgroups stay resident per CU
constexpr int kPqMaxP = 256;

struct PqCountParams {
  const int32_t* pred;     // [npix] of this image
  const void* gt;          // [npix] int32 (format 0) or [npix][3] uint8 RGB (format 1)
  int gt_format;
  int npix;
  int G, P;
  const int32_t* ids;      // [G] ascending declared ids
  int32_t* inter;          // [G + 2][P + 1] of this image
  int32_t* flags;          // the image's flags word
  int use_lds;
};

__device__ __forceinline__ int pq_row(const int32_t* s_ids, int G, int32_t id) {
  if (id == 0) return 0;
  int lo = 0, hi = G;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (s_ids[mid] < id) lo = mid + 1; else hi = mid;
  }
  return (lo < G && s_ids[lo] == id) ? lo + 1 : G + 1;
}

__global__ __launch_bounds__(kPqThreads) void pq_count_kernel(const PqCountParams p) {
  extern __shared__ int32_t s_mem[];
  int32_t* s_ids = s_mem;                      // [G]
  int32_t* s_tab = s_mem + p.G;                // [(G + 2) * (P + 1)] when use_lds
  const int W = p.P + 1;
  const int cells = (p.G + 2) * W;
  for (int i = threadIdx.x; i < p.G; i += kPqThreads) s_ids[i] = p.ids[i];
  if (p.use_lds)
    for (int i = threadIdx.x; i < cells; i += kPqThreads) s_tab[i] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int begin = blockIdx.x * kPqChunk;
  const int end = min(p.npix, begin + kPqChunk);
  bool bad_pred = false;
  for (int base = begin; base < end; base += kPqThreads) {      // uniform trip count: every lane reaches the shuffles
    const int i = base + threadIdx.x;
    int key = -1;
    if (i < end) {
      const int32_t q = p.pred[i];
      int32_t id;
      if (p.gt_format == 1) {
        const uint8_t* c = (const uint8_t*)p.gt + (size_t)i * 3;
        id = (int32_t)c[0] + 256 * (int32_t)c[1] + 65536 * (int32_t)c[2];
      } else {
        id = ((const int32_t*)p.gt)[i];
      }
      if (q < 0 || q > p.P) bad_pred = true;
      else key = pq_row(s_ids, p.G, id) * W + q;
    }
    // merge a run of equal neighbours into its first lane
    const int left = __shfl_up(key, 1);
    const bool head = lane == 0 || left != key;
    const unsigned long long heads = __ballot(head);
    if (head && key >= 0) {
      const unsigned long long rest = lane == 63 ? 0ull : heads >> (lane + 1);
      const int len = rest ? __ffsll((long long)rest) : 64 - lane;
      atomicAdd(p.use_lds ? &s_tab[key] : &p.inter[key], len);
    }
  }
  if (bad_pred) atomicOr(p.flags, 4);
  if (p.use_lds) {
    __syncthreads();
    for (int i = threadIdx.x; i < cells; i += kPqThreads)
      if (s_tab[i]) atomicAdd(&p.inter[i], s_tab[i]);
  }
}

// one workgroup per image
__global__ __launch_bounds__(kPqThreads) void pq_match_kernel(const int32_t* inter_all, const uint8_t* keep_all, const uint8_t* slot_crowd,
                                                              const int64_t* slot_area,
                                                              const int32_t* slot_meta, int P, int Gpad, int32_t* stats_all,
                                                              double* match_iou_all) {
  __shared__ int s_apred[kPqMaxP + 1];
  __shared__ long long s_agt[LDMSEG_PQ_G_MAX];
  __shared__ int s_gm[LDMSEG_PQ_G_MAX];
  __shared__ int s_pm[kPqMaxP + 1];
  __shared__ int s_cnt[4];                     // tp, fp, fn, flags
  const int b = blockIdx.x;
  const int W = P + 1;
  const int G = min(max(slot_meta[2 * b], 0), Gpad);
  const int last_crowd = slot_meta[2 * b + 1] < G ? slot_meta[2 * b + 1] : -1;
  const int32_t* inter = inter_all + (size_t)b * (Gpad + 2) * W;
  const uint8_t* keep = keep_all + (size_t)b * P;
  const uint8_t* crowd = slot_crowd + (size_t)b * Gpad;
  const int64_t* area = slot_area + (size_t)b * Gpad;
  double* match_iou = match_iou_all + (size_t)b * Gpad;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < 4) s_cnt[tid] = 0;
  for (int g = tid; g < Gpad; g += kPqThreads) { match_iou[g] = 0.0; s_gm[g] = 0; }
  // area of every prediction id: column sums over all G + 2 rows
  for (int q = tid; q < W; q += kPqThreads) {
    int a = 0;
    for (int r = 0; r < G + 2; ++r) a += inter[r * W + q];
    s_apred[q] = a;
    s_pm[q] = 0;
  }
  // area of every declared slot: the annotation's, or the counted one where it gives none (-1): a wave per row
  for (int g = wave; g < G; g += kPqThreads / 64) {
    long long a = area[g];
    if (a < 0) {
      int sum = 0;
      for (int q = lane; q < W; q += 64) sum += inter[(g + 1) * W + q];
      for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
      a = sum;
    }
    if (lane == 0) s_agt[g] = a;
  }
  __syncthreads();
  int flags = 0;
  for (int q = 1 + tid; q < W; q += kPqThreads) {
    const bool declared = keep[q - 1] != 0;
    if (s_apred[q] > 0 && !declared) flags |= 1;
    if (s_apred[q] == 0 && declared) flags |= 2;
  }
  // matching: every (declared non-crowd slot, declared prediction) pair that shares a pixel
  const int pairs = G * P;
  for (int i = tid; i < pairs; i += kPqThreads) {
    const int g = i / P, q = 1 + (i - g * P);
    const int n = inter[(g + 1) * W + q];
    if (n <= 0 || crowd[g] || !keep[q - 1]) continue;
    const long long uni = (long long)s_apred[q] + s_agt[g] - n - inter[q];
    if (uni < 0) continue;                           // a negative IoU matches nothing
    if (uni == 0) { flags |= 8; continue; }          // (Python divides by zero here: annotation areas that contradict the map)
    const double iou = (double)n / (double)uni;
    if (iou > 0.5) {
      atomicAdd(&s_cnt[0], 1);
      if (atomicAdd(&s_gm[g], 1) == 0) match_iou[g] = iou; else flags |= 8;
      if (atomicAdd(&s_pm[q], 1) != 0) flags |= 8;
    }
  }
  __syncthreads();
  int fn = 0, fp = 0;
  for (int g = tid; g < G; g += kPqThreads)
    if (!crowd[g] && s_gm[g] == 0) ++fn;
  for (int q = 1 + tid; q < W; q += kPqThreads) {
    if (!keep[q - 1] || s_pm[q] != 0 || s_apred[q] == 0) continue;
    long long ign = inter[q];
    if (last_crowd >= 0) ign += inter[(last_crowd + 1) * W + q];
    if ((double)ign / (double)s_apred[q] > 0.5) continue;
    ++fp;
  }
  if (fp) atomicAdd(&s_cnt[1], fp);
  if (fn) atomicAdd(&s_cnt[2], fn);
  if (flags) atomicOr(&s_cnt[3], flags);
  __syncthreads();
  int32_t* stats = stats_all + 4 * b;
  if (tid < 3) stats[tid] = s_cnt[tid];
  if (tid == 3 && s_cnt[3]) atomicOr(&stats[3], s_cnt[3]);   // pass A may have set bit 2 already
}

}  // namespace

// see ldmseg_pq_match (include/ldmseg_hip.h); sizes / pred_offsets / gt_offsets / gt_counts are HOST arrays
int launch_pq_match(const int32_t* pred, const void* gt, int gt_format, int B, const int32_t* sizes, const int64_t* pred_offsets,
                    const int64_t* gt_offsets, const uint8_t* keep, int P, const int32_t* gt_counts, int Gpad,
                    const int32_t* slot_ids, const uint8_t* slot_crowd, const int64_t* slot_area, const int32_t* slot_meta,
                    int32_t* inter, int32_t* stats, double* match_iou, hipStream_t s) {
  if (B < 1 || P < 1 || P > kPqMaxP || Gpad < 1 || Gpad > LDMSEG_PQ_G_MAX || (gt_format != 0 && gt_format != 1)) return -2;
  for (int b = 0; b < B; ++b) {
    if (gt_counts[b] < 0 || gt_counts[b] > Gpad || sizes[2 * b] < 1 || sizes[2 * b + 1] < 1) return -2;
    if ((int64_t)sizes[2 * b] * sizes[2 * b + 1] > (int64_t)0x7fff0000 || pred_offsets[b] < 0 || gt_offsets[b] < 0) return -2;
  }
  const size_t per = (size_t)(Gpad + 2) * (P + 1);
  if (hipMemsetAsync(inter, 0, (size_t)B * per * sizeof(int32_t), s) != hipSuccess) return -3;
  if (hipMemsetAsync(stats, 0, (size_t)B * 4 * sizeof(int32_t), s) != hipSuccess) return -3;
  for (int b = 0; b < B; ++b) {
    PqCountParams p;
    p.npix = sizes[2 * b] * sizes[2 * b + 1];
    p.pred = pred + pred_offsets[b];
    p.gt = gt_format == 1 ? (const void*)((const uint8_t*)gt + 3 * (size_t)gt_offsets[b])
                          : (const void*)((const int32_t*)gt + gt_offsets[b]);
    p.gt_format = gt_format;
    p.G = gt_counts[b]; p.P = P;
    p.ids = slot_ids + (size_t)b * Gpad;
    p.inter = inter + (size_t)b * per;
    p.flags = stats + 4 * b + 3;
    const size_t table = (size_t)(p.G + 2) * (P + 1) * sizeof(int32_t), ids = (size_t)p.G * sizeof(int32_t);
    p.use_lds = ids + table <= (size_t)kPqLdsBytes;
    const unsigned blocks = (unsigned)((p.npix + kPqChunk - 1) / kPqChunk);
    hipLaunchKernelGGL(pq_count_kernel, dim3(blocks), dim3(kPqThreads), p.use_lds ? ids + table : ids, s, p);
  }
  hipLaunchKernelGGL(pq_match_kernel, dim3(B), dim3(kPqThreads), 0, s, inter, keep, slot_crowd, slot_area, slot_meta, P, Gpad, stats,
                     match_iou);
  return launch_status();
}

}  // namespace ldmseg
