// 3dioumatch_amd/csrc/point_index.hip -- per-detection point lists: a stable multi-split of every
// scan's rows by an integer key (include/point_index_hip.h states the rule; votenet/point_index.py
// holds the host restatement).
//
// An LSD radix split, one digit of kBits bits per pass.  A pass is four launches:
//   count_kernel     grid (max_segments, S).  A workgroup counts the digits of its kSegment rows in LDS
//                    (integer LDS atomics: the counts do not depend on their order) and writes its
//                    row of the (scan, segment, digit) table, zeros included.
//   segments_kernel  one thread per (scan, digit) runs down the scan's segments: the count becomes the
//                    number of rows with that digit in EARLIER segments, the total goes to the bases.
//   digits_kernel    one workgroup per scan: an exclusive scan over the digits' totals, in place.
//                    In a single pass the digit is the bucket, so this is `start`.
//   scatter_kernel   grid (max_segments, S).  cursor[d] = base[d] + table[segment][d] in LDS; the
//                    segment is walked in order, kTile rows at a time.  Inside a wave the lanes with
//                    the same digit are found with one ballot per digit bit (a fixed number of steps
//                    whatever the keys: 64 distinct digits in a wave cost what one does) and ranked by
//                    lane; the lowest lane of each group moves the cursor on by the group's size.  The
//                    tile's waves do that one after the other with a barrier between them, so a row's
//                    position is cursor + (equal digits before it in the tile): the incoming order,
//                    whatever the timing.  The next tile's rows are loaded before the turns.
// With two passes (cap up to INDEX_MAX_CAP) pass 0 leaves its (bucket, index) pairs in the scratch, pass
// 1 also keeps the sorted buckets there, and boundary_kernel reads `start` off them: position p writes
// start[r] = p for every r in (bucket[p - 1], bucket[p]], position n the rest.  Every word of `start`
// has exactly one writer.
//
// No global atomics, no float atomics, no host read.  A key is only compared: a bad one falls into
// the tail bucket `cap`.
#include "common.h"
#include "../../include/point_index_hip.h"

namespace {

constexpr int kBits = INDEX_DIGIT_BITS;
constexpr int kDigits = 1 << kBits;
constexpr int kSegment = INDEX_SEGMENT;
constexpr int kTile = INDEX_TILE;
constexpr int kWaves = kTile / kWave;
static_assert(kSegment % kTile == 0 && kTile % kWave == 0, "whole tiles, whole waves");
constexpr int kBatch = 32;               // segments_kernel: table rows read ahead of their stores
constexpr int kPer = kDigits / kTile;    // digits_kernel: digits per thread at most
static_assert(kDigits % kTile == 0, "digits_kernel gives every thread the same number of digits");

inline int bits_of(unsigned v) {
  int b = 0;
  for (; v; v >>= 1) ++b;
  return b;
}
inline int passes_of(int cap) { return cap < kDigits ? 1 : 2; }  // cap <= INDEX_MAX_CAP
inline int digits_of(int cap, int pass) {
  const int top = (cap >> (kBits * pass)) + 1;
  return top < kDigits ? top : kDigits;
}

struct Layout {
  size_t table, base, pairs, bytes;  // byte offsets; pairs: 3 planes of P int32 (only with two passes)
};

inline Layout layout_of(int S, int cap, int max_segments, long long P) {
  const size_t d0 = (size_t)digits_of(cap, 0);
  Layout l;
  l.table = 0;
  l.base = l.table + 4 * (size_t)S * max_segments * d0;
  l.pairs = (l.base + 4 * (size_t)S * d0 + 7) / 8 * 8;
  l.bytes = (l.pairs + (passes_of(cap) > 1 ? 12 * (size_t)P : 0) + 7) / 8 * 8;
  return l;
}

struct Pass {
  int S, cap, max_segments;
  int shift, digits, digit_bits;  // this pass: key >> shift, digits < 2^digit_bits
  int single;                     // != 0: the only pass, digits_kernel writes start
  const int *key;                 // pass 0: the key plane; else nullptr
  const long long *offset;
  const int *count;
  const int *in_bucket, *in_index;  // later passes: what the pass before wrote
  int *out_bucket;                  // nullptr: not kept
  int *out_index;                   // a pair buffer, or order in the last pass
  int *table, *base, *start;
};

__device__ __forceinline__ int rows_of(const Pass &a, int scan) {
  const long long most = (long long)a.max_segments * kSegment;
  const long long n = a.count[scan];
  return (int)(n < 0 ? 0 : (n < most ? n : most));
}

__device__ __forceinline__ int bucket_at(const Pass &a, long long row) {
  if (!a.key) return a.in_bucket[row];
  const int k = a.key[row];
  return (unsigned)k < (unsigned)a.cap ? k : a.cap;  // -1 and every out-of-range key: the tail
}

__device__ __forceinline__ int digit_of(const Pass &a, int bucket) {
  return min((int)(((unsigned)bucket >> a.shift) & (unsigned)(kDigits - 1)), a.digits - 1);
}

// grid (max_segments, S)
__global__ void __launch_bounds__(kTile) count_kernel(const Pass a) {
  __shared__ int s_count[kDigits];
  const int scan = blockIdx.y, seg = blockIdx.x, t = threadIdx.x;
  const int n = rows_of(a, scan), first = seg * kSegment;
  if (first >= n) return;  // the whole workgroup; segments_kernel stops before this row
  for (int d = t; d < a.digits; d += kTile) s_count[d] = 0;
  __syncthreads();
  const int end = min(n, first + kSegment);
  const long long row0 = a.offset[scan];
  for (int j = first + t; j < end; j += kTile) atomicAdd(&s_count[digit_of(a, bucket_at(a, row0 + j))], 1);
  __syncthreads();
  int *row = a.table + ((size_t)scan * a.max_segments + seg) * a.digits;
  for (int d = t; d < a.digits; d += kTile) row[d] = s_count[d];
}

// grid (ceil(digits / kTile), S).  A thread's column is read kBatch segments at a time before the
// running counts are written back: the loads of a batch are in flight together (one load, one store
// per trip was 245 memory latencies in a row for a 1 M-point scan).
__global__ void __launch_bounds__(kTile) segments_kernel(const Pass a) {
  const int scan = blockIdx.y, d = blockIdx.x * kTile + threadIdx.x;
  if (d >= a.digits) return;
  const int segments = (rows_of(a, scan) + kSegment - 1) / kSegment;
  int *col = a.table + (size_t)scan * a.max_segments * a.digits + d;
  int run = 0;
  for (int seg0 = 0; seg0 < segments; seg0 += kBatch, col += (size_t)kBatch * a.digits) {
    int c[kBatch];
#pragma unroll
    for (int k = 0; k < kBatch; ++k) c[k] = seg0 + k < segments ? col[(size_t)k * a.digits] : 0;
#pragma unroll
    for (int k = 0; k < kBatch; ++k) {
      if (seg0 + k < segments) col[(size_t)k * a.digits] = run;
      run += c[k];
    }
  }
  a.base[(size_t)scan * a.digits + d] = run;
}

// grid (S): thread t owns the digits [t * per, (t + 1) * per), per <= kPer, read once into registers
__global__ void __launch_bounds__(kTile) digits_kernel(const Pass a) {
  __shared__ int s_wave[kWaves];
  const int scan = blockIdx.x, t = threadIdx.x, lane = lane_id(), wave = t / kWave;
  const int per = (a.digits + kTile - 1) / kTile;
  int *base = a.base + (size_t)scan * a.digits;
  const int d0 = t * per, d1 = min(d0 + per, a.digits);
  int c[kPer];
  int mine = 0;
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    c[k] = d0 + k < d1 ? base[d0 + k] : 0;
    mine += c[k];
  }
  int upto = mine;  // inclusive over the wave's lanes
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const int other = __shfl_up(upto, off, kWave);
    if (lane >= off) upto += other;
  }
  if (lane == kWave - 1) s_wave[wave] = upto;
  __syncthreads();
  int run = upto - mine;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) run += w < wave ? s_wave[w] : 0;
  int *start = a.start + (size_t)scan * ((size_t)a.cap + 1);
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    if (d0 + k < d1) {
      base[d0 + k] = run;
      if (a.single) start[d0 + k] = run;  // digits == cap + 1
    }
    run += c[k];
  }
}

// grid (max_segments, S)
__global__ void __launch_bounds__(kTile) scatter_kernel(const Pass a) {
  __shared__ int s_cursor[kDigits];
  const int scan = blockIdx.y, seg = blockIdx.x, t = threadIdx.x, wave = t / kWave;
  const int n = rows_of(a, scan), first = seg * kSegment;
  if (first >= n) return;  // the whole workgroup: no barrier is skipped by a part of it
  {
    const int *row = a.table + ((size_t)scan * a.max_segments + seg) * a.digits;
    const int *base = a.base + (size_t)scan * a.digits;
    for (int d = t; d < a.digits; d += kTile) s_cursor[d] = base[d] + row[d];
  }
  __syncthreads();
  const int end = min(n, first + kSegment);
  const long long row0 = a.offset[scan];
  const unsigned long long below = (1ull << lane_id()) - 1ull;
  int j = first + t;
  bool valid = j < end;
  int bucket = 0, index = 0;
  if (valid) {
    bucket = bucket_at(a, row0 + j);
    index = a.key ? j : a.in_index[row0 + j];
  }
  for (int j0 = first; j0 < end; j0 += kTile) {  // the same trip count for every thread
    const int jn = j + kTile;
    const bool validn = jn < end;
    int bucketn = 0, indexn = 0;
    if (validn) {  // the next tile's rows: in flight during the turns
      bucketn = bucket_at(a, row0 + jn);
      indexn = a.key ? jn : a.in_index[row0 + jn];
    }
    const int d = digit_of(a, bucket);
    unsigned long long same = __ballot(valid);
    for (int bit = 0; bit < a.digit_bits; ++bit) {
      const bool set = (d >> bit) & 1;
      const unsigned long long with = __ballot(set);
      same &= set ? with : ~with;
    }
    const int rank = __popcll(same & below), size = __popcll(same);
    int pos = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      if (wave == w && valid) {
        const int cursor = s_cursor[d];  // every lane of the group reads before its lowest lane writes
        pos = cursor + rank;
        if (rank == 0) s_cursor[d] = cursor + size;
      }
      __syncthreads();
    }
    if (valid) {
      if (a.out_bucket) a.out_bucket[row0 + pos] = bucket;
      a.out_index[row0 + pos] = index;
    }
    j = jn, valid = validn, bucket = bucketn, index = indexn;
  }
}

// grid (ceil((max_segments * kSegment + 1) / kTile), S): one thread per position 0..n of the sorted buckets
__global__ void __launch_bounds__(kTile) boundary_kernel(const Pass a, const int *sorted) {
  const int scan = blockIdx.y;
  const long long p = (long long)blockIdx.x * kTile + threadIdx.x;
  const int n = rows_of(a, scan);
  if (p > n) return;
  const long long row0 = a.offset[scan];
  const int before = p > 0 ? min(max(sorted[row0 + p - 1], 0), a.cap) : -1;
  const int here = p < n ? min(max(sorted[row0 + p], 0), a.cap) : a.cap;
  int *start = a.start + (size_t)scan * ((size_t)a.cap + 1);
  for (int r = before + 1; r <= here; ++r) start[r] = (int)p;
}

}  // namespace

PN2_API size_t scene_points_index_scratch_bytes(int S, int cap, int max_segments, long long P) {
  if (S < 1 || cap < 1 || cap > INDEX_MAX_CAP || max_segments < 1 || P < 0) return 0;
  return layout_of(S, cap, max_segments, P).bytes;
}

PN2_API int scene_points_index(const PointsIndexArgs *a, void *stream_) {
  if (!a || a->S < 1 || a->S > 65535 || a->cap < 1 || a->cap > INDEX_MAX_CAP || a->max_segments < 1 || a->P < 0 || !a->key || !a->offset ||
      !a->count || !a->start || !a->order || !a->scratch || ((uintptr_t)a->scratch & 7) != 0)
    return (int)hipErrorInvalidValue;
  const Layout l = layout_of(a->S, a->cap, a->max_segments, a->P);
  if (a->scratch_bytes < l.bytes) return (int)hipErrorInvalidValue;
  const long long positions = (long long)a->max_segments * kSegment + 1;
  if ((positions + kTile - 1) / kTile > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  hipStream_t stream = (hipStream_t)stream_;
  char *scratch = (char *)a->scratch;
  int *pairs = (int *)(scratch + l.pairs);
  int *bucket0 = pairs, *index0 = pairs + a->P, *sorted = pairs + 2 * a->P;  // read only with two passes
  const int passes = passes_of(a->cap);
  Pass p;
  p.S = a->S, p.cap = a->cap, p.max_segments = a->max_segments;
  p.single = passes == 1;
  p.offset = a->offset, p.count = a->count;
  p.table = (int *)(scratch + l.table), p.base = (int *)(scratch + l.base), p.start = a->start;
  const dim3 block(kTile), rows((unsigned)a->max_segments, (unsigned)a->S);
  for (int pass = 0; pass < passes; ++pass) {
    const bool last = pass == passes - 1;
    p.shift = kBits * pass;
    p.digits = digits_of(a->cap, pass);
    p.digit_bits = bits_of((unsigned)(p.digits - 1));
    p.key = pass == 0 ? a->key : nullptr;
    p.in_bucket = pass == 0 ? nullptr : bucket0;
    p.in_index = pass == 0 ? nullptr : index0;
    p.out_bucket = passes == 1 ? nullptr : (pass == 0 ? bucket0 : sorted);
    p.out_index = last ? a->order : index0;
    hipLaunchKernelGGL(count_kernel, rows, block, 0, stream, p);
    hipLaunchKernelGGL(segments_kernel, dim3((unsigned)((p.digits + kTile - 1) / kTile), (unsigned)a->S), block, 0,
                       stream, p);
    hipLaunchKernelGGL(digits_kernel, dim3((unsigned)a->S), block, 0, stream, p);
    hipLaunchKernelGGL(scatter_kernel, rows, block, 0, stream, p);
    if (last && passes > 1)
      hipLaunchKernelGGL(boundary_kernel, dim3((unsigned)((positions + kTile - 1) / kTile), (unsigned)a->S), block, 0,
                         stream, p, (const int *)sorted);
  }
  return (int)hipGetLastError();
}
