// 3dioumatch_amd/csrc/scan_tile.hip -- the tiled scan path (include/scan_tile_hip.h;
// votenet/scan_tiles.py and votenet/detect.py hold the host restatements).
//
//   tile_bounds_part_kernel  scans x (segments): min / max of x and y over one segment of a scan's
//   tile_bounds_kernel       rows, then per scan over its segments.  fminf / fmaxf in registers, a
//                            shuffle butterfly per wave, sixteen values through LDS: exact.
//   tile_count_kernel        tiles x (segments): the rows of one segment of the tile's parent that
//                            lie in the tile's window.  Every thread reads x and y of 64 rows.
//   tile_gather_kernel       tiles x (segments): the same rows, copied.  Stable compaction, 1024 rows
//                            per step: the lanes' votes as one ballot per wave, a lane's place
//                            among its wave's set bits (mask_rank), the waves' totals through LDS,
//                            and a running base that every thread carries in a register.
//   tile_merge_kernel        one workgroup per parent scan: tile by tile, 256 packed rows per step,
//                            the rows whose box centre lies in the tile's core -- compacted the same
//                            way into a list of source rows in LDS, from which all threads then copy
//                            the planes with consecutive addresses -- and zeros behind them.
//
// All five stream: no MFMA, no float atomics, one integer LDS atomic per wave in the count.
#include "common.h"
#include "../../include/scan_tile_hip.h"

#include <math.h>

namespace {

constexpr int kBlock = SCAN_TILE_BLOCK;
constexpr int kWaves = kBlock / kWave;
constexpr int kSeg = SCAN_TILE_SEGMENT;
constexpr int kMergeBlock = 256;
constexpr int kMergeWaves = kMergeBlock / kWave;

struct Extent {
  float xmin, xmax, ymin, ymax;
};

__device__ __forceinline__ Extent extent_empty() { return {INFINITY, -INFINITY, INFINITY, -INFINITY}; }

__device__ __forceinline__ void extent_add(Extent &e, float xmin, float xmax, float ymin, float ymax) {
  e.xmin = fminf(e.xmin, xmin);
  e.xmax = fmaxf(e.xmax, xmax);
  e.ymin = fminf(e.ymin, ymin);
  e.ymax = fmaxf(e.ymax, ymax);
}

// over the 64 lanes; every lane gets the result
__device__ __forceinline__ void extent_wave(Extent &e) {
#pragma unroll
  for (int off = kWave / 2; off >= 1; off >>= 1)
    extent_add(e, __shfl_xor(e.xmin, off, kWave), __shfl_xor(e.xmax, off, kWave), __shfl_xor(e.ymin, off, kWave),
               __shfl_xor(e.ymax, off, kWave));
}

__device__ __forceinline__ bool inside(const float4 w, float x, float y) {  // w: lo_x, hi_x, lo_y, hi_y
  return w.x <= x && x < w.y && w.z <= y && y < w.w;
}

__device__ __forceinline__ float4 load4(const float *p) { return make_float4(p[0], p[1], p[2], p[3]); }

__global__ void __launch_bounds__(kBlock) tile_bounds_part_kernel(const ScanBoundsArgs a) {
  __shared__ float s_part[kWaves][4];
  const int scan = blockIdx.x, seg = blockIdx.y, t = threadIdx.x, wave = t / kWave;
  const int n = a.count[scan], C = a.C;
  const int r0 = seg * kSeg;
  if (r0 >= n) return;  // not one of the scan's segments: its partial is never read
  const int r1 = min(n, r0 + kSeg);
  const float *rows = a.cloud + a.offset[scan] * C;
  Extent e = extent_empty();
  for (int i = r0 + t; i < r1; i += kBlock) {
    const float x = rows[(size_t)i * C], y = rows[(size_t)i * C + 1];
    extent_add(e, x, x, y, y);
  }
  extent_wave(e);
  if (lane_id() == 0) {
    s_part[wave][0] = e.xmin;
    s_part[wave][1] = e.xmax;
    s_part[wave][2] = e.ymin;
    s_part[wave][3] = e.ymax;
  }
  __syncthreads();
  if (t != 0) return;
  e = extent_empty();
  for (int w = 0; w < kWaves; ++w) extent_add(e, s_part[w][0], s_part[w][1], s_part[w][2], s_part[w][3]);
  float *out = a.partial + ((size_t)scan * a.max_segments + seg) * 4;
  out[0] = e.xmin;
  out[1] = e.xmax;
  out[2] = e.ymin;
  out[3] = e.ymax;
}

__global__ void __launch_bounds__(kWave) tile_bounds_kernel(const ScanBoundsArgs a) {
  const int scan = blockIdx.x, t = threadIdx.x;
  const int segments = min((a.count[scan] + kSeg - 1) / kSeg, a.max_segments);
  const float *part = a.partial + (size_t)scan * a.max_segments * 4;
  Extent e = extent_empty();
  for (int g = t; g < segments; g += kWave)
    extent_add(e, part[g * 4 + 0], part[g * 4 + 1], part[g * 4 + 2], part[g * 4 + 3]);
  extent_wave(e);
  if (t != 0) return;
  float *out = a.bounds + (size_t)scan * 4;
  out[0] = e.xmin;
  out[1] = e.xmax;
  out[2] = e.ymin;
  out[3] = e.ymax;
}

__global__ void __launch_bounds__(kBlock) tile_count_kernel(const ScanTileCountArgs a) {
  __shared__ int s_total;
  const int tile = blockIdx.x, seg = blockIdx.y, t = threadIdx.x;
  const int scan = a.parent[tile];
  const int n = a.count[scan], C = a.C;
  const int r0 = seg * kSeg;
  const int r1 = min(n, r0 + kSeg);  // r0 >= n: no rows, the entry is written as 0
  if (t == 0) s_total = 0;
  __syncthreads();
  const float4 w = load4(a.window + (size_t)tile * 4);
  const float *rows = a.cloud + a.offset[scan] * C;
  int mine = 0;
  for (int i = r0 + t; i < r1; i += kBlock)
    mine += inside(w, rows[(size_t)i * C], rows[(size_t)i * C + 1]) ? 1 : 0;
#pragma unroll
  for (int off = kWave / 2; off >= 1; off >>= 1) mine += __shfl_xor(mine, off, kWave);
  if (lane_id() == 0 && mine) atomicAdd(&s_total, mine);
  __syncthreads();
  if (t == 0) a.counts[(size_t)tile * a.max_segments + seg] = s_total;
}

__global__ void __launch_bounds__(kBlock) tile_gather_kernel(const ScanTileGatherArgs a) {
  __shared__ int s_wave[kWaves];
  const int tile = blockIdx.x, seg = blockIdx.y, t = threadIdx.x, wave = t / kWave;
  const int scan = a.parent[tile];
  const int n = a.count[scan], C = a.C;
  const int r0 = seg * kSeg;
  if (r0 >= n) return;
  const int r1 = min(n, r0 + kSeg);
  const float4 w = load4(a.window + (size_t)tile * 4);
  const float *rows = a.cloud + a.offset[scan] * C;
  long long base = a.base[(size_t)tile * a.max_segments + seg];
  for (int c0 = r0; c0 < r1; c0 += kBlock) {  // the same trip count for every thread
    const int i = c0 + t;
    const float *src = rows + (size_t)min(i, r1 - 1) * C;
    const bool in = i < r1 && inside(w, src[0], src[1]);
    const unsigned long long votes = __ballot(in);
    if (lane_id() == 0) s_wave[wave] = __popcll(votes);
    __syncthreads();
    int before = 0, step = 0;
#pragma unroll
    for (int v = 0; v < kWaves; ++v) {
      const int c = s_wave[v];
      before += v < wave ? c : 0;
      step += c;
    }
    const long long row = base + before + mask_rank(votes);
    if (in && row >= 0 && row < a.rows) {
      float *dst = a.crops + (size_t)row * C;
      if (C == 6) {
#pragma unroll
        for (int c = 0; c < 6; ++c) dst[c] = src[c];
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) dst[c] = src[c];
      }
    }
    base += step;
    __syncthreads();  // s_wave is rewritten by the next step
  }
}

__global__ void __launch_bounds__(kMergeBlock) tile_merge_kernel(const ScanMergeArgs a) {
  __shared__ int s_src[kMergeBlock];
  __shared__ int s_wave[kMergeWaves];
  const int s = blockIdx.x, t = threadIdx.x, wave = t / kWave;
  const int K = a.K, cap = a.cap, SW = a.NC > 0 ? a.NC : 1;
  const int tile0 = a.first[s], tile1 = tile0 + min(a.tiles[s], a.max_tiles);
  const size_t out0 = (size_t)s * cap;
  int total = 0;  // owned rows written so far: the same in every thread
  for (int tile = tile0; tile < tile1; ++tile) {
    const int c = min(max(a.count_in[tile], 0), K);
    const float4 core = load4(a.core + (size_t)tile * 4);
    const size_t in0 = (size_t)tile * K;
    for (int r0 = 0; r0 < c; r0 += kMergeBlock) {
      const int r = r0 + t;
      bool owned = false;
      if (r < c) {
        const float *b = a.box_in + (in0 + r) * 7;
        owned = inside(core, b[0], b[1]);
      }
      const unsigned long long votes = __ballot(owned);
      if (lane_id() == 0) s_wave[wave] = __popcll(votes);
      __syncthreads();
      int before = 0, step = 0;
#pragma unroll
      for (int v = 0; v < kMergeWaves; ++v) {
        const int n = s_wave[v];
        before += v < wave ? n : 0;
        step += n;
      }
      if (owned) s_src[before + mask_rank(votes)] = r;
      __syncthreads();
      step = min(step, cap - total);  // cap >= max_tiles * K: never cuts
      const size_t dst0 = out0 + total;
      for (int i = t; i < step; i += kMergeBlock) {
        const size_t k = in0 + s_src[i];
        a.tile[dst0 + i] = tile;
        a.proposal[dst0 + i] = a.proposal_in[k];
        a.cls[dst0 + i] = a.cls_in[k];
      }
      for (int i = t; i < step * SW; i += kMergeBlock) {
        const int j = i / SW, x = i - j * SW;
        a.score[dst0 * SW + i] = a.score_in[(in0 + s_src[j]) * SW + x];
      }
      for (int i = t; i < step * 7; i += kMergeBlock) {
        const int j = i / 7, x = i - j * 7;
        a.box[dst0 * 7 + i] = a.box_in[(in0 + s_src[j]) * 7 + x];
      }
      for (int i = t; i < step * 24; i += kMergeBlock) {
        const int j = i / 24, x = i - j * 24;
        a.corners[dst0 * 24 + i] = a.corners_in[(in0 + s_src[j]) * 24 + x];
      }
      total += step;
      __syncthreads();  // s_src and s_wave are rewritten by the next step
    }
  }
  if (t == 0) a.count[s] = total;
  const size_t end0 = out0 + total;
  const long long rest = cap - total;
  for (long long i = t; i < rest; i += kMergeBlock) {
    a.tile[end0 + i] = 0;
    a.proposal[end0 + i] = 0;
    a.cls[end0 + i] = 0;
  }
  for (long long i = t; i < rest * SW; i += kMergeBlock) a.score[end0 * SW + i] = 0.0f;
  for (long long i = t; i < rest * 7; i += kMergeBlock) a.box[end0 * 7 + i] = 0.0f;
  for (long long i = t; i < rest * 24; i += kMergeBlock) a.corners[end0 * 24 + i] = 0.0f;
}

inline bool bad_columns(int C) { return C != 3 && C != 6; }

}  // namespace

PN2_API int scene_scan_bounds(const ScanBoundsArgs *args, void *stream) {
  if (!args || args->S < 1 || bad_columns(args->C) || args->max_segments < 1 || !args->cloud || !args->offset ||
      !args->count || !args->partial || !args->bounds)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(tile_bounds_part_kernel, dim3(args->S, args->max_segments), dim3(kBlock), 0,
                     (hipStream_t)stream, *args);
  const int status = (int)hipGetLastError();
  if (status) return status;
  hipLaunchKernelGGL(tile_bounds_kernel, dim3(args->S), dim3(kWave), 0, (hipStream_t)stream, *args);
  return (int)hipGetLastError();
}

PN2_API int scene_scan_tile_count(const ScanTileCountArgs *args, void *stream) {
  if (!args || args->T < 1 || bad_columns(args->C) || args->max_segments < 1 || !args->cloud || !args->offset ||
      !args->count || !args->parent || !args->window || !args->counts)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(tile_count_kernel, dim3(args->T, args->max_segments), dim3(kBlock), 0, (hipStream_t)stream,
                     *args);
  return (int)hipGetLastError();
}

PN2_API int scene_scan_tile_gather(const ScanTileGatherArgs *args, void *stream) {
  if (!args || args->T < 1 || bad_columns(args->C) || args->max_segments < 1 || args->rows < 1 || !args->cloud ||
      !args->offset || !args->count || !args->parent || !args->window || !args->base || !args->crops)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(tile_gather_kernel, dim3(args->T, args->max_segments), dim3(kBlock), 0, (hipStream_t)stream,
                     *args);
  return (int)hipGetLastError();
}

PN2_API int scene_detections_merge(const ScanMergeArgs *args, void *stream) {
  if (!args || args->S < 1 || args->K < 1 || args->K > SCAN_MAX_K || args->NC < 0 || args->max_tiles < 1 ||
      (long long)args->cap < (long long)args->max_tiles * args->K || !args->first || !args->tiles || !args->core ||
      !args->count_in || !args->proposal_in || !args->cls_in || !args->score_in || !args->box_in ||
      !args->corners_in || !args->count || !args->tile || !args->proposal || !args->cls || !args->score ||
      !args->box || !args->corners)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(tile_merge_kernel, dim3(args->S), dim3(kMergeBlock), 0, (hipStream_t)stream, *args);
  return (int)hipGetLastError();
}
