// 3dioumatch_amd/csrc/point_labels.hip -- which packed detection owns each raw row of a scan store
// (include/point_labels_hip.h states the rule; votenet/point_labels.py holds the host restatement).
//
//   frames_kernel   one thread per (scan, row < cap): the row's frame in float64 rounded to float32
//                   (box_points.hip's), its 64-bit rank word (0: ineligible), cls and a bounding
//                   radius into the scratch, points[s, r] = 0.  Every word for all cap rows.
//   label_kernel    box_point_count_kernel transposed.  One lane per point, xyz in registers; the
//                   scan's rows pass through LDS kChunk at a time: thread t looks at row r0 + t, drops
//                   it if it is ineligible or (cull) its sphere misses the bounding box of the
//                   workgroup's points, and the survivors are compacted (ballot, lane rank, a scan
//                   over the waves) into two float4 and a rank per row.  Every lane then reads the
//                   same LDS address (a broadcast) and keeps the largest rank of the rows containing
//                   it: a maximum, so the staged order does not matter.  Per-pair arithmetic is
//                   float32, every operation rounded.
//
// The cull is exact.  A point the float32 test accepts has |dz| <= hh and fl(c dx - s dy),
// fl(s dx + c dy) within hl, hw, with dx = fl(px - cx) (relative error 2^-24), two rounded products and
// one rounded sum each (absolute error below 3 * 2^-24 * sqrt(2) * |d_xy|, plus 2^-148 where a product
// underflows) and c^2 + s^2 within 2^-22 of 1: its true distance from the centre is below
// sqrt(hl^2 + hw^2 + hh^2) * (1 + 2^-19) + 2^-140.  The radius is that root times (1 + 2^-10) plus
// 2^-120, in float64, rounded UP to float32; the distance from the centre to the workgroup's box and
// the comparison are float64 (relative error 2^-50).  A row is dropped only where that distance
// exceeds the radius, so no point of the workgroup can be inside it.
//
// `points` is only ever added to with agent-scope integer atomics; instance and semantic are plain
// vector stores of each lane's own word.  No float atomics, no host read.
#include "common.h"
#include "../../include/point_labels_hip.h"

#include <math.h>

namespace {

constexpr int kBlock = LABEL_BLOCK;
constexpr int kChunk = LABEL_BOX_CHUNK;
constexpr int kWaves = kBlock / kWave;
constexpr int kFramesBlock = 256;
constexpr int kBatch = 4;  // staged rows read from LDS ahead of their tests (divides the chunk)
static_assert(kChunk == kBlock, "a chunk is staged one row per thread");
static_assert(kChunk % kBatch == 0, "the padded tail stays inside the chunk");

struct Scratch {
  unsigned long long *rank;
  int *cls;
  float *radius;
};

__host__ __device__ inline Scratch scratch_of(const void *base, int S, int cap) {
  const size_t rows = (size_t)S * cap;
  unsigned long long *rank = (unsigned long long *)base;
  int *cls = (int *)(rank + rows);
  return {rank, cls, (float *)(cls + rows)};
}

inline size_t scratch_bytes(int S, int cap) { return S < 1 || cap < 1 ? 0 : (size_t)16 * S * cap; }

__device__ __forceinline__ bool finite32(float v) { return fabsf(v) < __int_as_float(0x7f800000); }

// grid ceil(S * cap / kFramesBlock)
__global__ void __launch_bounds__(kFramesBlock) frames_kernel(const DetectionsFramesArgs a) {
  const long long at = (long long)blockIdx.x * kFramesBlock + threadIdx.x;
  if (at >= (long long)a.S * a.cap) return;
  const int scan = (int)(at / a.cap), r = (int)(at % a.cap);
  const Scratch sc = scratch_of(a.scratch, a.S, a.cap);
  float *f = a.frames + (size_t)at * 8;
  a.points[at] = 0;
  const int count = min(max(a.count[scan], 0), a.cap);
  if (r >= count) {  // never read: zeros, owns nothing
#pragma unroll
    for (int k = 0; k < 8; ++k) f[k] = 0.f;
    sc.rank[at] = 0ull;
    sc.cls[at] = 0;
    sc.radius[at] = 0.f;
    return;
  }
  const float *b = a.box + (size_t)at * 7;
  const float l = b[3], w = b[4], h = b[5];
  const double ang = (double)b[6];
  const float c = (float)cos(ang), s = (float)sin(ang);
  const float cx = b[0], cy = b[1], cz = b[2];
  const float hl = (float)((double)l / 2), hw = (float)((double)w / 2), hh = (float)((double)h / 2);
  const float frame[8] = {c, s, cx, cy, cz, hl, hw, hh};
  const int cls = a.cls[at];
  sc.cls[at] = cls;
  bool ok = l > 0.f && w > 0.f && h > 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    f[k] = frame[k];
    ok = ok && finite32(frame[k]);
  }
  float key = 0.f;
  if (a.NC > 0) {
    if (cls >= 0 && cls < a.NC)
      key = a.score[(size_t)at * a.NC + cls];
    else
      ok = false;
  } else {
    key = a.score[at];
  }
  const double least = a.min_score > 0.0 ? a.min_score : 0.0;
  ok = ok && (double)key >= least;  // false for a NaN key
  unsigned long long rank = 0ull;
  float radius = 0.f;
  if (ok) {
    unsigned high;
    if (a.prefer == 0) {
      high = __float_as_uint(fabsf(key));
    } else {
      const float v = __fmul_rn(__fmul_rn(l, w), h);
      high = 0xFFFFFFFFu - __float_as_uint(v);
    }
    rank = ((unsigned long long)high << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)r);
    const double x = hl, y = hw, z = hh;
    const double reach = sqrt((x * x + y * y) + z * z) * (1.0 + 0x1p-10) + 0x1p-120;
    radius = (float)reach;
    if ((double)radius < reach) radius = __uint_as_float(__float_as_uint(radius) + 1u);  // round up
  }
  sc.rank[at] = rank;
  sc.radius[at] = radius;
}

// grid (max_blocks, S)
__global__ void __launch_bounds__(kBlock) label_kernel(const PointsLabelArgs a) {
  __shared__ float4 s_a[kChunk];  // c, s, cx, cy
  __shared__ float4 s_b[kChunk];  // cz, hl, hw, hh
  __shared__ unsigned long long s_rank[kChunk];
  __shared__ float s_box[kWaves][6];
  __shared__ int s_wave[kWaves];
  const int scan = blockIdx.y, t = threadIdx.x, wave = t / kWave;
  const int n = a.count[scan];
  const long long first = (long long)blockIdx.x * kBlock;
  if (first >= n) return;  // the whole workgroup: no barrier is skipped by a part of it
  const bool valid = first + t < n;
  const long long row = a.offset[scan] + first + t;
  const float nan = __int_as_float(0x7fc00000);
  float px = nan, py = nan, pz = nan;  // a NaN point is inside no box
  if (valid) {
    const float *p = a.cloud + (size_t)row * a.C;
    px = p[0], py = p[1], pz = p[2];
  }
  const int rows = min(max(a.rows[scan], 0), a.cap);
  const size_t base = (size_t)scan * a.cap;
  const Scratch sc = scratch_of(a.scratch, a.S, a.cap);

  double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  if (a.cull) {  // the bounding box of the workgroup's points (fminf / fmaxf skip a NaN)
    const float inf = __int_as_float(0x7f800000);
    float v[6] = {valid ? px : inf, valid ? py : inf, valid ? pz : inf,
                  valid ? px : -inf, valid ? py : -inf, valid ? pz : -inf};
#pragma unroll
    for (int off = kWave / 2; off >= 1; off >>= 1) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        v[k] = fminf(v[k], __shfl_xor(v[k], off, kWave));
        v[3 + k] = fmaxf(v[3 + k], __shfl_xor(v[3 + k], off, kWave));
      }
    }
    if (lane_id() == 0) {
#pragma unroll
      for (int k = 0; k < 6; ++k) s_box[wave][k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float l = s_box[0][k], h = s_box[0][3 + k];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) {
        l = fminf(l, s_box[w][k]);
        h = fmaxf(h, s_box[w][3 + k]);
      }
      lo[k] = l, hi[k] = h;
    }
  }

  unsigned long long best = 0ull;
  for (int r0 = 0; r0 < rows; r0 += kChunk) {  // the same trip count for every thread
    const int r = r0 + t;
    unsigned long long rank = 0ull;
    float f[8];
    bool keep = false;
    if (r < rows) {
      rank = sc.rank[base + r];
      keep = rank != 0ull;
    }
    if (keep) {
      const float *src = a.frames + (base + r) * 8;
#pragma unroll
      for (int k = 0; k < 8; ++k) f[k] = src[k];
      if (a.cull) {
        const double radius = sc.radius[base + r];
        double d2 = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double c = f[2 + k];
          const double e = fmax(fmax(lo[k] - c, c - hi[k]), 0.0);
          d2 += e * e;
        }
        keep = !(d2 > radius * radius);  // a NaN keeps the row
      }
    }
    const unsigned long long votes = __ballot(keep);
    if (lane_id() == 0) s_wave[wave] = __popcll(votes);
    __syncthreads();
    int before = 0, staged = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const int c = s_wave[w];
      before += w < wave ? c : 0;
      staged += c;
    }
    if (keep) {
      const int slot = before + mask_rank(votes);
      s_a[slot] = make_float4(f[0], f[1], f[2], f[3]);
      s_b[slot] = make_float4(f[4], f[5], f[6], f[7]);
      s_rank[slot] = rank;
    }
    // the tail up to a multiple of kBatch is padded with NaN frames: they contain no point
    const int padded = (staged + kBatch - 1) / kBatch * kBatch;
    if (t < padded - staged) {
      s_a[staged + t] = make_float4(nan, nan, nan, nan);
      s_b[staged + t] = make_float4(nan, nan, nan, nan);
      s_rank[staged + t] = 0ull;
    }
    __syncthreads();
    for (int k0 = 0; k0 < padded; k0 += kBatch) {
      float4 u[kBatch], v[kBatch];  // all the batch's LDS reads in flight before the first use
#pragma unroll
      for (int k = 0; k < kBatch; ++k) u[k] = s_a[k0 + k], v[k] = s_b[k0 + k];
#pragma unroll
      for (int k = 0; k < kBatch; ++k) {
        const float dx = __fsub_rn(px, u[k].z), dy = __fsub_rn(py, u[k].w), dz = __fsub_rn(pz, v[k].x);
        const float xr = __fsub_rn(__fmul_rn(u[k].x, dx), __fmul_rn(u[k].y, dy));
        const float zr = __fadd_rn(__fmul_rn(u[k].y, dx), __fmul_rn(u[k].x, dy));
        // `&`, not `&&`: three compares and two mask ands, no branch per compare
        const int inside = (int)(fabsf(xr) <= v[k].y) & (int)(fabsf(zr) <= v[k].z) & (int)(fabsf(dz) <= v[k].w);
        if (inside) {  // rare: the rank is read only then
          const unsigned long long rk = s_rank[k0 + k];
          best = rk > best ? rk : best;
        }
      }
    }
    __syncthreads();  // the staged rows and s_wave are rewritten by the next chunk
  }

  int owner = best ? (int)(0xFFFFFFFFu - (unsigned)best) : -1;
  if (owner >= rows) owner = -1;  // only with a scratch the frames launch did not write
  if (valid) {
    a.instance[row] = owner;
    a.semantic[row] = owner >= 0 ? sc.cls[base + owner] : -1;
  }
  // one atomic per distinct owner of the wave
  unsigned long long left = __ballot(valid && owner >= 0);
  while (left) {
    const int leader = __ffsll((long long)left) - 1;
    const int theirs = __shfl(owner, leader, kWave);
    const unsigned long long same = __ballot(owner == theirs) & left;
    if (lane_id() == leader)
      __hip_atomic_fetch_add(a.points + base + owner, __popcll(same), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    left &= ~same;
  }
}

inline bool bad_scratch(const void *scratch, size_t bytes, int S, int cap) {
  return !scratch || ((uintptr_t)scratch & 7) != 0 || bytes < scratch_bytes(S, cap);
}

}  // namespace

PN2_API size_t scene_points_label_scratch_bytes(int S, int cap) { return scratch_bytes(S, cap); }

PN2_API int scene_detections_frames(const DetectionsFramesArgs *a, void *stream) {
  if (!a || a->S < 1 || a->S > 65535 || a->K < 1 || a->K > SCAN_MAX_K || a->cap < 1 || a->NC < 0 ||
      (a->prefer != 0 && a->prefer != 1) || !isfinite(a->min_score) || !a->count || !a->cls || !a->score || !a->box ||
      !a->frames || !a->points || bad_scratch(a->scratch, a->scratch_bytes, a->S, a->cap))
    return (int)hipErrorInvalidValue;
  const long long blocks = ((long long)a->S * a->cap + kFramesBlock - 1) / kFramesBlock;
  if (blocks > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(frames_kernel, dim3((unsigned)blocks), dim3(kFramesBlock), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}

PN2_API int scene_points_label(const PointsLabelArgs *a, void *stream) {
  if (!a || a->S < 1 || a->S > 65535 || (a->C != 3 && a->C != 6) || a->K < 1 || a->K > SCAN_MAX_K || a->cap < 1 ||
      a->max_blocks < 1 || !a->cloud || !a->offset || !a->count || !a->rows || !a->frames || !a->instance ||
      !a->semantic || !a->points || bad_scratch(a->scratch, a->scratch_bytes, a->S, a->cap))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(label_kernel, dim3((unsigned)a->max_blocks, (unsigned)a->S), dim3(kBlock), 0,
                     (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}
