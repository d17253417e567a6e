// 3dioumatch_amd/csrc/scannet_raw.hip -- raw ScanNet scans -> the four arrays of the preprocessed
// layout (include/scannet_raw_hip.h; votenet/scannet_raw.py holds the readers, the seg tables, the
// host validation and the numpy restatement).
//
//   raw_extent_init_kernel  the empty extents: min keys all ones, max keys zero.  No finite float has
//                           the key zero, so a zero max key afterwards says "no vertex".
//   raw_extent_kernel       one thread per vertex of the chunk.  The thread finds its scan in the
//                           offset table (a workgroup, even a wave, may straddle two scans), aligns
//                           its vertex and looks its object up.  The lanes of a wave that share an
//                           object reduce their six keys by a butterfly and ONE lane issues the six
//                           global integer atomics; the loop runs once per distinct object of the
//                           wave, and a mesh's vertex order keeps that number small.  min and max do
//                           not depend on order: the extents are deterministic.
//   raw_box_kernel          one workgroup per scan, one thread per object: centre and size in float32
//                           (numpy on float32 scalars), the 18-class filter, an ordered compaction by
//                           wave ballots and a prefix over the waves' totals.
//   raw_rows_kernel         one thread per output row: the kept vertex (identity, the draw of
//                           csrc/scene_common.h, or a given choice), aligned again by the function
//                           raw_extent_kernel aligns with, and the two table lookups.
#include "common.h"
#include "scene_common.h"
#include "../../include/scannet_raw_hip.h"

namespace {

constexpr int kBlock = 256;
constexpr int kBoxBlock = SNR_MAX_OBJECTS;
constexpr int kBoxWaves = kBoxBlock / kWave;
// OBJ_CLASS_IDS (batch_load_scannet_data.py:35) as a bit set: 3 4 5 6 7 8 9 10 11 12 14 16 24 28 33 34 36 39
constexpr unsigned long long kObjClassBits =
    (1ull << 3) | (1ull << 4) | (1ull << 5) | (1ull << 6) | (1ull << 7) | (1ull << 8) | (1ull << 9) |
    (1ull << 10) | (1ull << 11) | (1ull << 12) | (1ull << 14) | (1ull << 16) | (1ull << 24) |
    (1ull << 28) | (1ull << 33) | (1ull << 34) | (1ull << 36) | (1ull << 39);

// the scan whose rows hold row i: the largest s with off[s] <= i (every scan has a row)
__device__ __forceinline__ int find_scan(const long long *off, int S, long long i) {
  int lo = 0, hi = S - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= i) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// row r of [x y z 1] . M^T as load_scannet_data.py:78-81 has it: float64 products summed left to
// right, nothing fused, then the store into the float32 vertex array
__device__ __forceinline__ float align_row(const double *m, double x, double y, double z) {
  double acc = __dmul_rn(x, m[0]);
  acc = __dadd_rn(acc, __dmul_rn(y, m[1]));
  acc = __dadd_rn(acc, __dmul_rn(z, m[2]));
  acc = __dadd_rn(acc, __dmul_rn(1.0, m[3]));
  return (float)acc;
}

__device__ __forceinline__ void align_point(const double *m, const float *raw, float &x, float &y, float &z) {
  const double dx = raw[0], dy = raw[1], dz = raw[2];
  x = align_row(m + 0, dx, dy, dz);
  y = align_row(m + 4, dx, dy, dz);
  z = align_row(m + 8, dx, dy, dz);
}

__device__ __forceinline__ unsigned wave_min_u32(unsigned v) {
#pragma unroll
  for (int off = kWave / 2; off >= 1; off >>= 1) v = min(v, (unsigned)__shfl_xor((int)v, off, kWave));
  return v;
}

__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
#pragma unroll
  for (int off = kWave / 2; off >= 1; off >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, off, kWave));
  return v;
}

__global__ void __launch_bounds__(kBlock) raw_extent_init_kernel(unsigned *extent, long long words) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i < words) extent[i] = (i % 6) < 3 ? 0xFFFFFFFFu : 0u;
}

__global__ void __launch_bounds__(kBlock) raw_extent_kernel(const ScanNetRawArgs a) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  int object = -1;  // the vertex's row of `extent` (T < 2^31); -1: no object, or a thread past the end
  float x = 0.0f, y = 0.0f, z = 0.0f;
  if (i < a.P) {
    const int s = find_scan(a.vert_offset, a.S, i);
    align_point(a.matrix + (size_t)s * 16, a.raw + (size_t)i * 6, x, y, z);
    const int o = a.seg_object[a.seg_offset[s] + a.seg[i]];
    if (o > 0) object = (int)a.obj_offset[s] + (o - 1);
  }
  const unsigned kx = order_key(x), ky = order_key(y), kz = order_key(z);
  // every lane of the wave runs the loop (its condition is the same in all of them): the shuffles
  // below read all 64 lanes
  unsigned long long todo = __ballot(object >= 0);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int lead = __shfl(object, leader, kWave);
    const bool mine = object == lead;
    const unsigned lx = wave_min_u32(mine ? kx : 0xFFFFFFFFu), hx = wave_max_u32(mine ? kx : 0u);
    const unsigned ly = wave_min_u32(mine ? ky : 0xFFFFFFFFu), hy = wave_max_u32(mine ? ky : 0u);
    const unsigned lz = wave_min_u32(mine ? kz : 0xFFFFFFFFu), hz = wave_max_u32(mine ? kz : 0u);
    if (lane_id() == leader) {
      unsigned *e = a.extent + (size_t)lead * 6;
      atomicMin(e + 0, lx);
      atomicMin(e + 1, ly);
      atomicMin(e + 2, lz);
      atomicMax(e + 3, hx);
      atomicMax(e + 4, hy);
      atomicMax(e + 5, hz);
    }
    todo &= ~__ballot(mine);
  }
}

__global__ void __launch_bounds__(kBoxBlock) raw_box_kernel(const ScanNetRawArgs a) {
  __shared__ int s_wave[kBoxWaves];
  const int s = blockIdx.x, t = threadIdx.x, wave = t / kWave;
  const long long base = a.obj_offset[s];
  const int objects = (int)(a.obj_offset[s + 1] - base);  // <= SNR_MAX_OBJECTS = the workgroup
  bool kept = false;
  int label = 0;
  float cx = 0.0f, cy = 0.0f, cz = 0.0f, dx = 0.0f, dy = 0.0f, dz = 0.0f;
  if (t < objects) {
    const unsigned *e = a.extent + (size_t)(base + t) * 6;
    if (e[3] != 0u) {  // an object without vertices stays an all-zero row: label 0, not kept (:105)
      const float xmin = from_order_key(e[0]), ymin = from_order_key(e[1]), zmin = from_order_key(e[2]);
      const float xmax = from_order_key(e[3]), ymax = from_order_key(e[4]), zmax = from_order_key(e[5]);
      cx = __fdiv_rn(__fadd_rn(xmin, xmax), 2.0f);
      cy = __fdiv_rn(__fadd_rn(ymin, ymax), 2.0f);
      cz = __fdiv_rn(__fadd_rn(zmin, zmax), 2.0f);
      dx = __fsub_rn(xmax, xmin);
      dy = __fsub_rn(ymax, ymin);
      dz = __fsub_rn(zmax, zmin);
      label = a.object_label[base + t];
      kept = label >= 0 && label < 64 && ((kObjClassBits >> label) & 1ull);
    }
  }
  const unsigned long long votes = __ballot(kept);
  if (lane_id() == 0) s_wave[wave] = __popcll(votes);
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < kBoxWaves; ++w) {
    const int c = s_wave[w];
    before += w < wave ? c : 0;
    total += c;
  }
  if (kept) {
    double *row = a.bbox + (size_t)(base + before + mask_rank(votes)) * 7;
    row[0] = cx;
    row[1] = cy;
    row[2] = cz;
    row[3] = dx;
    row[4] = dy;
    row[5] = dz;
    row[6] = (double)label;
  }
  if (t == 0) a.nbox[s] = total;
}

__global__ void __launch_bounds__(kBlock) raw_rows_kernel(const ScanNetRawArgs a) {
  const long long q = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (q >= a.Q) return;
  const int s = find_scan(a.out_offset, a.S, q);
  const long long first = a.vert_offset[s];
  const int n = (int)(a.vert_offset[s + 1] - first), j = (int)(q - a.out_offset[s]);
  const int keep = a.keep[s];
  int p = j;  // SNR_KEEP_ALL: DONOTCARE_CLASS_IDS is empty in the reference, its mask the identity
  if (keep == SNR_KEEP_GIVEN) {
    p = a.choice[q];
  } else if (keep == SNR_KEEP_DRAWN) {
    const unsigned key = draw_key(a.seed, 0u, (unsigned)a.scan_index[s], SB_DRAW_STUDENT);
    p = sample_index(key, j, n, a.max_points, feistel_half_bits(n));
  }
  const float *raw = a.raw + (size_t)(first + p) * 6;
  float x, y, z;
  align_point(a.matrix + (size_t)s * 16, raw, x, y, z);
  float *out = a.vert + (size_t)q * 6;
  out[0] = x;
  out[1] = y;
  out[2] = z;
  out[3] = raw[3];
  out[4] = raw[4];
  out[5] = raw[5];
  const long long entry = a.seg_offset[s] + a.seg[first + p];
  a.ins_label[q] = (unsigned)a.seg_object[entry];
  a.sem_label[q] = (unsigned)a.seg_label[entry];
}

}  // namespace

PN2_API int scannet_raw_export(const ScanNetRawArgs *args, void *stream) {
  const long long limit = 0x7FFFFFFFll;
  if (!args || args->S < 1 || args->P < args->S || args->P > limit || args->Q < args->S || args->Q > args->P ||
      args->T < 0 || args->T > limit || args->max_points < 1 || args->max_objects < 0 || args->max_objects > SNR_MAX_OBJECTS ||
      !args->raw || !args->seg || !args->matrix || !args->vert_offset || !args->seg_offset ||
      !args->seg_label || !args->seg_object || !args->obj_offset || !args->object_label ||
      !args->out_offset || !args->keep || !args->scan_index || !args->extent || !args->vert ||
      !args->ins_label || !args->sem_label || !args->bbox || !args->nbox)
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  if (args->T > 0) {
    const long long words = args->T * 6;
    hipLaunchKernelGGL(raw_extent_init_kernel, dim3(pn2_ceil_div(words, kBlock)), dim3(kBlock), 0, st,
                       args->extent, words);
    hipLaunchKernelGGL(raw_extent_kernel, dim3(pn2_ceil_div(args->P, kBlock)), dim3(kBlock), 0, st, *args);
  }
  hipLaunchKernelGGL(raw_box_kernel, dim3(args->S), dim3(kBoxBlock), 0, st, *args);
  hipLaunchKernelGGL(raw_rows_kernel, dim3(pn2_ceil_div(args->Q, kBlock)), dim3(kBlock), 0, st, *args);
  return (int)hipGetLastError();
}
