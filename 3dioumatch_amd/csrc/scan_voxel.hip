// 3dioumatch_amd/csrc/scan_voxel.hip -- voxel-grid downsample of scan stores (include/scan_voxel_hip.h;
// votenet/scan_voxels.py holds the host restatement).
//
//   voxel_clear_kernel    every key and best word of the table to all ones, the scans' out-of-range
//                         counters to 0.
//   voxel_insert_kernel   one thread per row: its cell, the cell's slot in the scan's open-addressing
//                         table (64-bit compare-and-swap on the key word, linear probe), a 64-bit minimum
//                         of the row's rank on the slot's best word, the slot kept per row.
//   voxel_count_kernel    scans x (segments): the rows whose rank is their slot's best word.
//   voxel_gather_kernel   scans x (segments): the same rows, copied -- tile_gather_kernel's stable
//                         compaction (scan_tile.hip) with "kept" in place of "inside the window".
//
// The insert touches the table through agent-scope 64-bit atomics only and decides on what the swap
// returned: a plain load of a word another workgroup writes in the same launch may be stale (the XCDs'
// L2s are not coherent).  Which thread claims a slot varies from run to run; the set of keys and the
// minimum per key do not, and count and gather read the table only through each row's own slot.  No
// float atomics: the float64 distance of `nearest` is rounded to float32 and compared as its bits.
#include "common.h"
#include "../../include/scan_voxel_hip.h"

#include <math.h>

namespace {

constexpr int kBlock = SCAN_TILE_BLOCK;
constexpr int kWaves = kBlock / kWave;
constexpr int kSeg = SCAN_TILE_SEGMENT;
constexpr int kInsertBlock = 256;
constexpr int kClearBlock = 256;
constexpr double kLimit = (double)SCAN_VOXEL_CELL_LIMIT;
constexpr unsigned long long kEmpty = ~0ull;

__host__ __device__ inline long long voxel_slots(int count) {
  if (count < 1 || count >= (1 << 30)) return 0;
  long long n = 2;
  while (n < 2ll * count) n <<= 1;
  return n;
}

// The run of scan `scan`: its first slot and its size, 0 where the run does not lie inside the scratch.
struct Run {
  long long first, slots;
};

__device__ __forceinline__ Run voxel_run(const ScanVoxelArgs &a, int scan) {
  const long long first = a.slot_offset[scan], n = voxel_slots(a.count[scan]);
  const bool ok = n > 0 && first >= 0 && first <= a.total_slots - n;
  return {first, ok ? n : 0};
}

// The cell of the row at p as three floored float64 quotients; false where it is out of range
// (a NaN compares false and is out of range too).
__device__ __forceinline__ bool voxel_cell(const ScanVoxelArgs &a, const float *p, double c[3]) {
  bool ok = true;
#pragma unroll
  for (int x = 0; x < 3; ++x) {
    c[x] = floor((double)p[x] / a.voxel[x]);
    ok = ok && fabs(c[x]) < kLimit;
  }
  return ok;
}

__device__ __forceinline__ unsigned long long voxel_key(const double c[3]) {
  const long long half = SCAN_VOXEL_CELL_LIMIT;
  return ((unsigned long long)((long long)c[2] + half) << 42) | ((unsigned long long)((long long)c[1] + half) << 21) |
         (unsigned long long)((long long)c[0] + half);
}

// The rank of row i of its scan, in its cell c (read only with `nearest`).
__device__ __forceinline__ unsigned long long voxel_rank(const ScanVoxelArgs &a, const float *p, const double c[3],
                                                         int i) {
  if (!a.nearest) return (unsigned long long)(unsigned)i;
  double d[3];
#pragma unroll
  for (int x = 0; x < 3; ++x) d[x] = (double)p[x] - (c[x] + 0.5) * a.voxel[x];
  const float d2 = (float)((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
  return ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)i;
}

// splitmix64's finaliser
__device__ __forceinline__ unsigned long long voxel_mix(unsigned long long k) {
  k ^= k >> 30;
  k *= 0xbf58476d1ce4e5b9ull;
  k ^= k >> 27;
  k *= 0x94d049bb133111ebull;
  k ^= k >> 31;
  return k;
}

__global__ void __launch_bounds__(kClearBlock) voxel_clear_kernel(const ScanVoxelArgs a) {
  unsigned long long *words = (unsigned long long *)a.scratch;
  const long long n = 2 * a.total_slots, stride = (long long)gridDim.x * kClearBlock;
  const long long t = (long long)blockIdx.x * kClearBlock + threadIdx.x;
  for (long long i = t; i < n; i += stride) words[i] = kEmpty;
  if (t < a.S) a.outside[t] = 0;
}

// grid (max_segments * kSeg / kInsertBlock, S)
__global__ void __launch_bounds__(kInsertBlock) voxel_insert_kernel(const ScanVoxelArgs a) {
  const int scan = blockIdx.y;
  const long long at = (long long)blockIdx.x * kInsertBlock + threadIdx.x;
  const int n = a.count[scan];
  if (at >= n) return;
  const int i = (int)at;
  const long long row = a.offset[scan] + i;
  const float *p = a.cloud + (size_t)row * a.C;
  const Run run = voxel_run(a, scan);
  double c[3];
  if (!voxel_cell(a, p, c) || run.slots == 0) {
    atomicAdd(&a.outside[scan], 1);
    a.slot[row] = -1;
    return;
  }
  const unsigned long long key = voxel_key(c), rank = voxel_rank(a, p, c, i);
  unsigned long long *keys = (unsigned long long *)a.scratch + run.first;
  unsigned long long *best = (unsigned long long *)a.scratch + a.total_slots + run.first;
  const unsigned long long mask = (unsigned long long)run.slots - 1;
  unsigned long long h = voxel_mix(key) & mask;
  int found = -1;
  // at most half the run is ever claimed, so the probe ends at an empty slot; the bound is for a
  // table that was not cleared
  for (long long probe = 0; probe < run.slots; ++probe) {
    unsigned long long seen = kEmpty;
    __hip_atomic_compare_exchange_strong(keys + h, &seen, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
    if (seen == kEmpty || seen == key) {  // `seen`: what the swap found there
      found = (int)h;
      break;
    }
    h = (h + 1) & mask;
  }
  if (found < 0) {
    atomicAdd(&a.outside[scan], 1);
    a.slot[row] = -1;
    return;
  }
  __hip_atomic_fetch_min(best + found, rank, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  a.slot[row] = found;
}

// row i of the scan whose rows begin at `row0` is kept: a launch boundary lies behind the insert, so
// these are plain loads
__device__ __forceinline__ bool voxel_kept(const ScanVoxelArgs &a, const Run &run, long long row0, int i) {
  const int s = a.slot[row0 + i];
  if (s < 0 || s >= run.slots) return false;
  const unsigned long long won = ((const unsigned long long *)a.scratch)[a.total_slots + run.first + s];
  if (!a.nearest) return won == (unsigned long long)(unsigned)i;
  const float *p = a.cloud + (size_t)(row0 + i) * a.C;
  double c[3];
  return voxel_cell(a, p, c) && won == voxel_rank(a, p, c, i);
}

__global__ void __launch_bounds__(kBlock) voxel_count_kernel(const ScanVoxelCountArgs b) {
  __shared__ int s_total;
  const ScanVoxelArgs &a = b.mark;
  const int scan = blockIdx.x, seg = blockIdx.y, t = threadIdx.x;
  const int n = a.count[scan];
  const int r0 = seg * kSeg;
  const int r1 = min(n, r0 + kSeg);  // r0 >= n: no rows, the entry is written as 0
  if (t == 0) s_total = 0;
  __syncthreads();
  const Run run = voxel_run(a, scan);
  const long long row0 = a.offset[scan];
  int mine = 0;
  for (int i = r0 + t; i < r1; i += kBlock) mine += voxel_kept(a, run, row0, i) ? 1 : 0;
#pragma unroll
  for (int off = kWave / 2; off >= 1; off >>= 1) mine += __shfl_xor(mine, off, kWave);
  if (lane_id() == 0 && mine) atomicAdd(&s_total, mine);
  __syncthreads();
  if (t == 0) b.counts[(size_t)scan * a.max_segments + seg] = s_total;
}

__global__ void __launch_bounds__(kBlock) voxel_gather_kernel(const ScanVoxelGatherArgs b) {
  __shared__ int s_wave[kWaves];
  const ScanVoxelArgs &a = b.mark;
  const int scan = blockIdx.x, seg = blockIdx.y, t = threadIdx.x, wave = t / kWave;
  const int n = a.count[scan], C = a.C;
  const int r0 = seg * kSeg;
  if (r0 >= n) return;
  const int r1 = min(n, r0 + kSeg);
  const Run run = voxel_run(a, scan);
  const long long row0 = a.offset[scan];
  long long base = b.base[(size_t)scan * a.max_segments + seg];
  for (int c0 = r0; c0 < r1; c0 += kBlock) {  // the same trip count for every thread
    const int i = c0 + t;
    const bool in = i < r1 && voxel_kept(a, run, row0, i);
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
    if (in && row >= 0 && row < b.rows) {
      const float *src = a.cloud + (size_t)(row0 + i) * C;
      float *dst = b.out + (size_t)row * C;
      if (C == 6) {
#pragma unroll
        for (int c = 0; c < 6; ++c) dst[c] = src[c];
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) dst[c] = src[c];
      }
      b.source[row] = i;
    }
    base += step;
    __syncthreads();  // s_wave is rewritten by the next step
  }
}

inline bool bad_mark(const ScanVoxelArgs *a) {
  if (!a || a->S < 1 || a->S > 65535 || (a->C != 3 && a->C != 6) || a->max_segments < 1 ||
      a->max_segments > 65535 || a->total_slots < 1 || !a->cloud || !a->offset || !a->count || !a->slot_offset ||
      !a->scratch || !a->slot || !a->outside || ((uintptr_t)a->scratch & 7) != 0)
    return true;
  for (int x = 0; x < 3; ++x)
    if (!(a->voxel[x] > 0) || !isfinite(a->voxel[x])) return true;
  return a->total_slots > (long long)(a->scratch_bytes / 16);
}

}  // namespace

PN2_API long long scene_scan_voxel_slots(int count) { return voxel_slots(count); }

PN2_API int scene_scan_voxel_mark(const ScanVoxelArgs *args, void *stream) {
  if (bad_mark(args)) return (int)hipErrorInvalidValue;
  const hipStream_t st = (hipStream_t)stream;
  const long long words = 2 * args->total_slots;
  long long blocks = (words + kClearBlock - 1) / kClearBlock;
  const long long least = (args->S + kClearBlock - 1) / kClearBlock;  // a thread per counter
  blocks = blocks > 8192 ? 8192 : blocks;
  blocks = blocks < least ? least : blocks;
  hipLaunchKernelGGL(voxel_clear_kernel, dim3((unsigned)blocks), dim3(kClearBlock), 0, st, *args);
  const int status = (int)hipGetLastError();
  if (status) return status;
  const dim3 grid((unsigned)args->max_segments * (kSeg / kInsertBlock), args->S);
  hipLaunchKernelGGL(voxel_insert_kernel, grid, dim3(kInsertBlock), 0, st, *args);
  return (int)hipGetLastError();
}

PN2_API int scene_scan_voxel_count(const ScanVoxelCountArgs *args, void *stream) {
  if (!args || bad_mark(&args->mark) || !args->counts) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(voxel_count_kernel, dim3(args->mark.S, args->mark.max_segments), dim3(kBlock), 0,
                     (hipStream_t)stream, *args);
  return (int)hipGetLastError();
}

PN2_API int scene_scan_voxel_gather(const ScanVoxelGatherArgs *args, void *stream) {
  if (!args || bad_mark(&args->mark) || args->rows < 1 || !args->base || !args->out || !args->source)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(voxel_gather_kernel, dim3(args->mark.S, args->mark.max_segments), dim3(kBlock), 0,
                     (hipStream_t)stream, *args);
  return (int)hipGetLastError();
}
