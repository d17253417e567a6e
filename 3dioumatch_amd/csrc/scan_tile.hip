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
//   seam_rows_kernel         scene_detections_merge_nms, the merge with an NMS across the cuts: per packed
//   seam_partners_kernel     row its flags, bounds, area and key; per candidate its partners in the up to
//   seam_resolve_kernel      eight tiles next to its own; per scan the winners, in rounds bounded by the
//   seam_write_kernel        undecided rows; and tile_merge_kernel's compaction of the kept rows.
//
// The first five stream: no MFMA, no float atomics, one integer LDS atomic per wave in the count.  The
// seam's overlaps are float64 in nms_aabb_block_kernel's expression order (lhs_nms.hip).
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

// ---- the seam: scene_detections_merge_nms ------------------------------------------------------------
constexpr int kSeamBlock = 256;
constexpr int kResolveBlock = 1024;
constexpr int kPartBlock = 512;  // seam_partners_kernel: its waves share 64 rows
constexpr int kPartWaves = kPartBlock / kWave;
constexpr int kPartners = SCAN_SEAM_PARTNERS;
constexpr int kCandidate = 1, kOwned = 2;  // bits of SeamScratch::flags

// The planes of the scratch.  A row is (scan * max_tiles + tile of the scan) * K + packed row, so
// every index below stays inside S * max_tiles * K rows whatever `first` holds.
struct SeamScratch {
  double *area;   // (rows,)
  float *bounds;  // (rows, 6) x1, y1, z1, x2, y2, z2
  float *key;     // (rows,)
  int *flags;     // (rows,) kCandidate | kOwned; 0 for a row at or past the tile's count
  int *partners;  // (rows,) partners of a candidate
  int *above;     // (rows,) those ordered above it
  int *first;     // (rows, kPartners) the first of them: rows of the scan, (tile of the scan) * K + packed row
  int *state;     // (rows,) of a candidate: 0 undecided, else 2 * (round + 1) + won
};
constexpr size_t kSeamRowBytes = sizeof(double) + 4 * (6 + 1 + 1 + 1 + 1 + kPartners + 1);

__host__ __device__ inline SeamScratch seam_scratch(void *p, size_t rows) {
  SeamScratch w;
  w.area = (double *)p;
  w.bounds = (float *)(w.area + rows);
  w.key = w.bounds + rows * 6;
  w.flags = (int *)(w.key + rows);
  w.partners = w.flags + rows;
  w.above = w.partners + rows;
  w.first = w.above + rows;
  w.state = w.first + rows * kPartners;
  return w;
}

__device__ __forceinline__ SeamScratch seam_scratch(const ScanSeamArgs &a) {
  return seam_scratch(a.scratch, (size_t)a.S * a.max_tiles * a.K);
}

struct SeamRow {
  float x1, y1, z1, x2, y2, z2, key;
  double area;
  int cls, tile, r;
};

__device__ __forceinline__ SeamRow seam_load(const ScanSeamArgs &a, const SeamScratch &w, size_t row, int tile, int r) {
  const float *b = w.bounds + row * 6;
  return {b[0], b[1], b[2], b[3], b[4], b[5], w.key[row], w.area[row], a.cls_in[(size_t)tile * a.K + r], tile, r};
}

// p comes before q: key descending, then tile, then packed row ascending
__device__ __forceinline__ bool seam_above(const SeamRow &p, const SeamRow &q) {
  return p.key > q.key || (p.key == q.key && (p.tile < q.tile || (p.tile == q.tile && p.r < q.r)));
}

// nms_aabb_block_kernel's test (lhs_nms.hip), `hi` the row ordered above `lo`.  Boxes that are apart
// along an axis leave before the float64 part where the threshold is >= 0: their intersection is 0, the
// overlap 0 / x is 0 or NaN, and neither is above it.  The float32 compare decides that exactly (a
// difference of two float32 values in float64 is > 0 iff the first is the larger).  Boxes of two
// tiles that are metres apart end there; the bench's random-weight boxes are large and mostly meet, and
// the exit still took the partners launch from 0.58 ms to 0.52 ms on 16 tiles x 256 candidates.
__device__ __forceinline__ bool seam_overlap(const ScanSeamArgs &a, const SeamRow &hi, const SeamRow &lo) {
  const float x1 = hi.x1 > lo.x1 ? hi.x1 : lo.x1, y1 = hi.y1 > lo.y1 ? hi.y1 : lo.y1,
              z1 = hi.z1 > lo.z1 ? hi.z1 : lo.z1;
  const float x2 = hi.x2 < lo.x2 ? hi.x2 : lo.x2, y2 = hi.y2 < lo.y2 ? hi.y2 : lo.y2,
              z2 = hi.z2 < lo.z2 ? hi.z2 : lo.z2;
  if (a.thresh >= 0 && (!(x2 > x1) || !(z2 > z1) || (a.dims != 2 && !(y2 > y1)))) return false;
  const double xx1 = x1, yy1 = y1, zz1 = z1, xx2 = x2, yy2 = y2, zz2 = z2;
  const double l = xx2 - xx1 > 0 ? xx2 - xx1 : 0, wd = yy2 - yy1 > 0 ? yy2 - yy1 : 0,
               h = zz2 - zz1 > 0 ? zz2 - zz1 : 0;
  const double inter = a.dims == 2 ? l * h : l * wd * h;
  double o = a.old_type ? inter / lo.area : inter / (hi.area + lo.area - inter);
  if (a.same_class) o = o * (hi.cls == lo.cls ? 1.0 : 0.0);
  return o > a.thresh;
}

// f(row of the scan, ordered above `me`) for every partner of `me`, tile `lt` of scan s: the
// candidates of the scan's other tiles next to it in the grid, tiles and rows ascending.  One thread
// on its own: the resolve's rescan of a row with more partners above it than it recorded.
template <class F>
__device__ __forceinline__ void seam_for_partners(const ScanSeamArgs &a, const SeamScratch &w, int s, int lt,
                                                  const SeamRow &me, F f) {
  const int K = a.K, tile0 = a.first[s], nt = min(a.tiles[s], a.max_tiles);
  const int iy = a.iy[me.tile], ix = a.ix[me.tile];
  const size_t scan0 = (size_t)s * a.max_tiles * K;
  for (int u = 0; u < nt; ++u) {
    const int other = tile0 + u;
    if (u == lt || abs(a.iy[other] - iy) > 1 || abs(a.ix[other] - ix) > 1) continue;
    const int c = min(max(a.count_in[other], 0), K);
    for (int j = 0; j < c; ++j) {
      const int q = u * K + j;
      if (!(w.flags[scan0 + q] & kCandidate)) continue;
      const SeamRow p = seam_load(a, w, scan0 + q, other, j);
      const bool above = seam_above(p, me);
      if (above ? seam_overlap(a, p, me) : seam_overlap(a, me, p)) f(q, above);
    }
  }
}

// grid (S, max_tiles, ceil(K / kSeamBlock)): one thread per packed row
__global__ void __launch_bounds__(kSeamBlock) seam_rows_kernel(const ScanSeamArgs a) {
  const int s = blockIdx.x, lt = blockIdx.y, r = blockIdx.z * kSeamBlock + threadIdx.x, K = a.K;
  if (lt >= min(a.tiles[s], a.max_tiles) || r >= K) return;
  const int tile = a.first[s] + lt;
  const SeamScratch w = seam_scratch(a);
  const size_t row = ((size_t)s * a.max_tiles + lt) * K + r, in = (size_t)tile * K + r;
  int flags = 0;
  if (r < min(max(a.count_in[tile], 0), K)) {
    const float *b = a.box_in + in * 7;
    if (inside(load4(a.reach + (size_t)tile * 4), b[0], b[1]))
      flags = kCandidate | (inside(load4(a.core + (size_t)tile * 4), b[0], b[1]) ? kOwned : 0);
  }
  w.flags[row] = flags;
  if (!flags) return;  // nothing else of the row is read
  const float *c = a.corners_in + in * 24;
  float lo[3] = {c[0], c[1], c[2]}, hi[3] = {c[0], c[1], c[2]};
#pragma unroll
  for (int k = 1; k < 8; ++k)
#pragma unroll
    for (int x = 0; x < 3; ++x) {
      const float v = c[k * 3 + x];
      if (v < lo[x]) lo[x] = v;
      if (v > hi[x]) hi[x] = v;
    }
  float *out = w.bounds + row * 6;
#pragma unroll
  for (int x = 0; x < 3; ++x) {
    out[x] = lo[x];
    out[3 + x] = hi[x];
  }
  w.area[row] = a.dims == 2 ? ((double)hi[0] - lo[0]) * ((double)hi[2] - lo[2])
                            : ((double)hi[0] - lo[0]) * ((double)hi[1] - lo[1]) * ((double)hi[2] - lo[2]);
  // the arg-max class is in 0..NC-1 by construction; the clamp only keeps a foreign arena's read in bounds
  w.key[row] = a.NC > 0 ? a.score_in[in * a.NC + min(max(a.cls_in[in], 0), a.NC - 1)] : a.score_in[in];
}

// grid (S, max_tiles, ceil(K / 64)): a workgroup is 64 packed rows of one tile, held by each of its
// kPartWaves waves (lane = row).  seam_for_partners' walk, spread out: the candidates of a neighbouring
// tile are compacted into LDS, kPartBlock packed rows per step (tile_gather_kernel's ballot and
// rank), and wave v then takes entries v, v + kPartWaves, .. of that list, every lane reading the
// same entry; the waves' counts and their first partners above each row meet in LDS at the end.
// Why: the pair test is a chain of dependent float64 instructions, a division among them, and 16
// tiles x 256 candidates are only 64 waves' worth of rows.  Measured on that case
// (profiles/detect_tiled_seam.json): a thread per candidate walking the neighbours' rows in global
// memory 0.79 ms, one wave per 64 rows over the LDS list 0.58 ms, with seam_overlap's early exit
// 0.52 ms, this form 0.09 ms.
__global__ void __launch_bounds__(kPartBlock) seam_partners_kernel(const ScanSeamArgs a) {
  __shared__ SeamRow s_row[kPartBlock];
  __shared__ int s_wave[kPartWaves];
  __shared__ int s_partners[kPartWaves][kWave], s_above[kPartWaves][kWave], s_first[kPartWaves][kWave][kPartners];
  const int s = blockIdx.x, lt = blockIdx.y, t = threadIdx.x, wave = t / kWave, lane = lane_id(), K = a.K;
  const int r = blockIdx.z * kWave + lane, nt = min(a.tiles[s], a.max_tiles);
  if (lt >= nt) return;
  const SeamScratch w = seam_scratch(a);
  const int tile0 = a.first[s], tile = tile0 + lt;
  const size_t scan0 = (size_t)s * a.max_tiles * K, row = scan0 + (size_t)lt * K + r;
  const bool candidate = r < K && (w.flags[row] & kCandidate);
  if (!__syncthreads_or(candidate)) return;  // the same answer in every thread
  SeamRow me = {};
  if (candidate) me = seam_load(a, w, row, tile, r);
  const int iy = a.iy[tile], ix = a.ix[tile];
  int partners = 0, above = 0;  // of this wave's share of the lists
  for (int u = 0; u < nt; ++u) {
    const int other = tile0 + u;
    if (u == lt || abs(a.iy[other] - iy) > 1 || abs(a.ix[other] - ix) > 1) continue;
    const int c = min(max(a.count_in[other], 0), K);
    for (int j0 = 0; j0 < c; j0 += kPartBlock) {  // the same trip count for every thread
      const int j = j0 + t;
      const size_t q = scan0 + (size_t)u * K + j;
      const bool in = j < c && (w.flags[q] & kCandidate);
      const unsigned long long votes = __ballot(in);
      if (lane == 0) s_wave[wave] = __popcll(votes);
      __syncthreads();
      int before = 0, n = 0;
#pragma unroll
      for (int v = 0; v < kPartWaves; ++v) {
        const int m = s_wave[v];
        before += v < wave ? m : 0;
        n += m;
      }
      if (in) s_row[before + mask_rank(votes)] = seam_load(a, w, q, other, j);
      __syncthreads();
      if (candidate) {
        for (int k = wave; k < n; k += kPartWaves) {
          const SeamRow p = s_row[k];
          const bool is_above = seam_above(p, me);
          if (!(is_above ? seam_overlap(a, p, me) : seam_overlap(a, me, p))) continue;
          ++partners;
          if (!is_above) continue;
          if (above < kPartners) s_first[wave][lane][above] = u * K + p.r;
          ++above;
        }
      }
      __syncthreads();  // s_row and s_wave are rewritten by the next step
    }
  }
  s_partners[wave][lane] = partners;
  s_above[wave][lane] = above;
  __syncthreads();
  if (wave != 0 || !candidate) return;
  // A row with at most kPartners partners above it has them all in the waves' lists: the resolve needs
  // every one of them, in any order.  With more it rescans, and what is recorded is not read.
  int all = 0, all_above = 0, kept = 0;
  for (int v = 0; v < kPartWaves; ++v) {
    all += s_partners[v][lane];
    const int n = s_above[v][lane];
    all_above += n;
    for (int k = 0; k < min(n, kPartners) && kept < kPartners; ++k)
      w.first[row * kPartners + kept++] = s_first[v][lane][k];
  }
  w.partners[row] = all;
  w.above[row] = all_above;
  w.state[row] = all_above ? 0 : 3;  // nothing above it: a winner of round 0
}

// one workgroup per scan
__global__ void __launch_bounds__(kResolveBlock) seam_resolve_kernel(const ScanSeamArgs a) {
  __shared__ int s_left;
  const int s = blockIdx.x, t = threadIdx.x, K = a.K;
  const int n = min(a.tiles[s], a.max_tiles) * K;
  const SeamScratch w = seam_scratch(a);
  const size_t scan0 = (size_t)s * a.max_tiles * K;
  const int *flags = w.flags + scan0;
  volatile int *state = w.state + scan0;  // written and read by this workgroup only, across its barriers
  int mine = 0;  // this thread's undecided rows
  for (int i = t; i < n; i += kResolveBlock) mine += (flags[i] & kCandidate) && state[i] == 0 ? 1 : 0;
  if (t == 0) s_left = 0;
  __syncthreads();
  if (mine) atomicAdd(&s_left, mine);
  __syncthreads();
  const int undecided = s_left;
  // Round `round` reads only what rounds < round decided (the tag in the state), so the outcome of a
  // round does not depend on the order of its threads.  The highest undecided row has all its
  // partners above it decided, so every round decides a row: at most `undecided` rounds.
  for (int round = 1; round <= undecided; ++round) {
    __syncthreads();  // every thread has read s_left
    if (t == 0) s_left = 0;
    __syncthreads();
    if (mine) {
      int still = 0;
      for (int i = t; i < n; i += kResolveBlock) {
        if (!(flags[i] & kCandidate) || state[i] != 0) continue;
        bool lost = false, open = false;
        auto see = [&](int st) {
          if (st != 0 && (st >> 1) <= round)
            lost = lost || (st & 1);
          else
            open = true;
        };
        const int above = w.above[scan0 + i];
        if (above <= kPartners) {
          for (int k = 0; k < above; ++k) see(state[w.first[(scan0 + i) * kPartners + k]]);
        } else {
          const int lt = i / K, r = i - lt * K;
          const SeamRow me = seam_load(a, w, scan0 + i, a.first[s] + lt, r);
          seam_for_partners(a, w, s, lt, me, [&](int q, bool is_above) {
            if (is_above) see(state[q]);
          });
        }
        if (lost)
          state[i] = 2 * (round + 1);
        else if (!open)
          state[i] = 2 * (round + 1) + 1;
        else
          ++still;
      }
      mine = still;
      if (still) atomicAdd(&s_left, still);
    }
    __threadfence_block();
    __syncthreads();
    if (s_left == 0) break;  // the same word in every thread
  }
}

// tile_merge_kernel with "kept" in place of "owned"
__global__ void __launch_bounds__(kMergeBlock) seam_write_kernel(const ScanSeamArgs a) {
  __shared__ int s_src[kMergeBlock];
  __shared__ int s_wave[kMergeWaves];
  const int s = blockIdx.x, t = threadIdx.x, wave = t / kWave;
  const int K = a.K, cap = a.cap, SW = a.NC > 0 ? a.NC : 1;
  const int tile0 = a.first[s], nt = min(a.tiles[s], a.max_tiles);
  const SeamScratch w = seam_scratch(a);
  const size_t out0 = (size_t)s * cap;
  int total = 0;  // kept rows written so far: the same in every thread
  for (int lt = 0; lt < nt; ++lt) {
    const int tile = tile0 + lt;
    const int c = min(max(a.count_in[tile], 0), K);
    const size_t in0 = (size_t)tile * K, row0 = ((size_t)s * a.max_tiles + lt) * K;
    for (int r0 = 0; r0 < c; r0 += kMergeBlock) {
      const int r = r0 + t;
      bool kept = false;
      if (r < c) {
        const int f = w.flags[row0 + r];
        kept = (f & kCandidate) && (w.state[row0 + r] & 1) && ((f & kOwned) || w.partners[row0 + r] > 0);
      }
      const unsigned long long votes = __ballot(kept);
      if (lane_id() == 0) s_wave[wave] = __popcll(votes);
      __syncthreads();
      int before = 0, step = 0;
#pragma unroll
      for (int v = 0; v < kMergeWaves; ++v) {
        const int n = s_wave[v];
        before += v < wave ? n : 0;
        step += n;
      }
      if (kept) s_src[before + mask_rank(votes)] = r;
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

PN2_API size_t scene_detections_merge_nms_scratch_bytes(int S, int T, int K, int max_tiles) {
  if (S < 1 || T < 1 || K < 1 || max_tiles < 1) return 0;
  return (size_t)S * max_tiles * K * kSeamRowBytes;
}

PN2_API int scene_detections_merge_nms(const ScanSeamArgs *args, void *stream) {
  if (!args || args->S < 1 || args->K < 1 || args->K > SCAN_MAX_K || args->NC < 0 || args->max_tiles < 1 ||
      args->max_tiles > SCAN_TILE_MAX || (long long)args->cap < (long long)args->max_tiles * args->K ||
      (args->dims != 2 && args->dims != 3) || (args->dims == 2 && args->same_class) || !args->first ||
      !args->tiles || !args->core || !args->count_in || !args->proposal_in || !args->cls_in || !args->score_in ||
      !args->box_in || !args->corners_in || !args->count || !args->tile || !args->proposal || !args->cls ||
      !args->score || !args->box || !args->corners || !args->iy || !args->ix || !args->reach || !args->scratch ||
      ((uintptr_t)args->scratch & 7) != 0 ||
      args->scratch_bytes < scene_detections_merge_nms_scratch_bytes(args->S, 1, args->K, args->max_tiles))
    return (int)hipErrorInvalidValue;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 rows(args->S, args->max_tiles, (args->K + kSeamBlock - 1) / kSeamBlock);
  hipLaunchKernelGGL(seam_rows_kernel, rows, dim3(kSeamBlock), 0, st, *args);
  int status = (int)hipGetLastError();
  if (status) return status;
  const dim3 chunks(args->S, args->max_tiles, (args->K + kWave - 1) / kWave);
  hipLaunchKernelGGL(seam_partners_kernel, chunks, dim3(kPartBlock), 0, st, *args);
  if ((status = (int)hipGetLastError())) return status;
  hipLaunchKernelGGL(seam_resolve_kernel, dim3(args->S), dim3(kResolveBlock), 0, st, *args);
  if ((status = (int)hipGetLastError())) return status;
  hipLaunchKernelGGL(seam_write_kernel, dim3(args->S), dim3(kMergeBlock), 0, st, *args);
  return (int)hipGetLastError();
}
