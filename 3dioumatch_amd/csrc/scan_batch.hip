// 3dioumatch_amd/csrc/scan_batch.hip -- the label-free scan path (include/scan_hip.h;
// votenet/scan_data.py and votenet/detect.py hold the host restatements).
//
//   scan_prepare_kernel   one workgroup per scan, once per store: the count of non-finite values and
//                         the floor height np.percentile(z, 0.99).  The two order statistics numpy
//                         interpolates are selected EXACTLY: four 8-bit radix passes over the
//                         order-preserving integer image of z find the key of rank lo, how many
//                         points share it and where lo falls among them; rank lo + 1 is the same key
//                         when it still falls among them and the smallest larger key (one more pass)
//                         otherwise.  Then numpy's float32 lerp, every operation rounded.
//   scan_batch_kernel     (chunks of 2048 sample slots) x rows: the sample index of each slot (the
//                         draw SB_DRAW_STUDENT of csrc/scene_common.h, as the labeled loaders' eval
//                         batches), the gathered raw row, the colour normalisation rounded once from
//                         double and height = z - floor.
//   scan_semi_kernel      (chunks of 2048 sample slots) x unlabeled rows x (student, teacher): the
//                         unlabeled rows of a semi-supervised batch from raw clouds.  The slot's row
//                         as scan_batch_kernel makes it (draws SB_DRAW_STUDENT / SB_DRAW_EMA of the
//                         row's place in the whole batch, row0 + r), SUN RGB-D's colour / 256 in
//                         float32, and for the student the dataset's flip / rotate / scale: the
//                         functions of csrc/scene_common.h that scene_points_kernel and
//                         sun_points_kernel call (row_aug, aug_point), not a copy of them.  All eight
//                         gathers of a thread are issued before the first is used.  One thread per
//                         row writes the header with the labeled box kernels' write_row_header.
//                         Both halves' rows are eval_row below, as scan_batch_kernel's are.
//   scan_pack_kernel      one workgroup per scene: the kept proposals ranked by (objectness
//                         probability descending, proposal ascending) with pseudo_rank::rank, then
//                         every plane of the scene's arena rows written in row order -- rows past
//                         the count as zeros, so the arena needs no clear.
#include "common.h"
#include "scene_common.h"
#include "pseudo_rank.h"
#include "../../include/scan_hip.h"

namespace {

constexpr int kPrepBlock = 1024;
constexpr int kPrepWaves = kPrepBlock / kWave;
constexpr int kBlock = 256;
constexpr int kPerThread = 8;
constexpr int kChunk = kBlock * kPerThread;  // sample slots per workgroup of scan_batch_kernel

__global__ void __launch_bounds__(kPrepBlock) scan_prepare_kernel(const ScanPrepareArgs a) {
  __shared__ unsigned s_hist[kPrepWaves * 256];  // one histogram per wave: less contention
  __shared__ unsigned s_tot[256];
  __shared__ unsigned s_prefix, s_rank, s_equal, s_bad, s_next;
  const int scan = blockIdx.x, t = threadIdx.x, wave = t / kWave;
  const int n = a.count[scan], C = a.C;
  const float *rows = a.cloud + a.offset[scan] * C;
  if (t == 0) {
    s_bad = 0u;
    s_next = 0xFFFFFFFFu;
  }
  __syncthreads();
  unsigned bad = 0u;
  const long long total = (long long)n * C;
  for (long long i = t; i < total; i += kPrepBlock) bad += isfinite(rows[i]) ? 0u : 1u;
  if (bad) atomicAdd(&s_bad, bad);

  // numpy's virtual index of the linear method in float32: (n - 1) * (f32(0.99) / f32(100))
  constexpr float q = 0.99f / 100.0f;
  const float v = __fmul_rn(q, (float)(n - 1));
  const int lo = min((int)floorf(v), n - 1);
  const int hi = min(lo + 1, n - 1);
  const float g = __fsub_rn(v, (float)lo);

  unsigned prefix = 0u, mask = 0u, rank = (unsigned)lo;
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int i = t; i < kPrepWaves * 256; i += kPrepBlock) s_hist[i] = 0u;
    __syncthreads();
    for (int i = t; i < n; i += kPrepBlock) {
      const unsigned key = order_key(rows[(size_t)i * C + 2]);
      if ((key & mask) == prefix) atomicAdd(&s_hist[wave * 256 + ((key >> shift) & 255u)], 1u);
    }
    __syncthreads();
    if (t < 256) {
      unsigned s = 0u;
      for (int w = 0; w < kPrepWaves; ++w) s += s_hist[w * 256 + t];
      s_tot[t] = s;
    }
    __syncthreads();
    if (t == 0) {
      unsigned cum = 0u;
      int d = 0;
      for (; d < 255; ++d) {
        if (rank < cum + s_tot[d]) break;
        cum += s_tot[d];
      }
      s_prefix = prefix | ((unsigned)d << shift);
      s_rank = rank - cum;
      s_equal = s_tot[d];
    }
    __syncthreads();
    prefix = s_prefix;
    rank = s_rank;
    mask |= 255u << shift;
  }
  // prefix: the key of rank lo; s_equal points share it and lo is number `rank` of them
  const bool same = hi == lo || rank + 1u < s_equal;
  if (!same) {
    unsigned next = 0xFFFFFFFFu;
    for (int i = t; i < n; i += kPrepBlock) {
      const unsigned key = order_key(rows[(size_t)i * C + 2]);
      if (key > prefix && key < next) next = key;
    }
    if (next != 0xFFFFFFFFu) atomicMin(&s_next, next);
  }
  __syncthreads();
  if (t != 0) return;
  const float lower = from_order_key(prefix);
  const float upper = (same || s_next == 0xFFFFFFFFu) ? lower : from_order_key(s_next);
  // numpy.lib._function_base_impl._lerp: a + (b - a) t, and b - (b - a)(1 - t) where t >= 0.5
  const float diff = __fsub_rn(upper, lower);
  a.floor[scan] = g >= 0.5f ? __fsub_rn(upper, __fmul_rn(diff, __fsub_rn(1.0f, g)))
                            : __fadd_rn(lower, __fmul_rn(diff, g));
  a.nonfinite[scan] = (int)min(s_bad, 0x7FFFFFFFu);
}

// Raw row (x y z [r g b]) -> the eval row of the dataset's detection loader, e = x y z r g b height:
// xyz as stored, the colour normalisation rounded once from double (without `color` no colour
// column is read), height = z - floor.
__device__ __forceinline__ void eval_row(bool sun, bool color, const float *raw, float floor, float (&e)[7]) {
  e[0] = raw[0];
  e[1] = raw[1];
  e[2] = raw[2];
  e[3] = e[4] = e[5] = 0.0f;
  if (color) {
    if (sun) {  // rgb - MEAN_COLOR_RGB, 0.5 each
#pragma unroll
      for (int c = 3; c < 6; ++c) e[c] = (float)((double)raw[c] - 0.5);
    } else {  // (rgb - MEAN_COLOR_RGB) / 256.0
      e[3] = (float)(((double)raw[3] - 109.8) / 256.0);
      e[4] = (float)(((double)raw[4] - 97.2) / 256.0);
      e[5] = (float)(((double)raw[5] - 83.8) / 256.0);
    }
  }
  e[6] = __fsub_rn(raw[2], floor);
}

// the row's channels in output order: xyz, [rgb], [height]
__device__ __forceinline__ void store_row(float *dst, bool color, bool height, const float (&e)[7]) {
  dst[0] = e[0];
  dst[1] = e[1];
  dst[2] = e[2];
  if (color) {
    dst[3] = e[3];
    dst[4] = e[4];
    dst[5] = e[5];
  }
  if (height) dst[color ? 6 : 3] = e[6];
}

__global__ void __launch_bounds__(kBlock) scan_batch_kernel(const ScanBatchArgs a) {
  const int chunk = blockIdx.x, row = blockIdx.y, t = threadIdx.x;
  const int scene = a.scene[row];
  const int n = a.count[scene], N = a.N, C = a.C;
  const bool color = a.use_color != 0, height = a.use_height != 0;
  const bool sun = a.dataset == SCAN_DATASET_SUNRGBD;
  const int OC = 3 + (color ? 3 : 0) + (height ? 1 : 0);
  if (chunk == 0 && t == 0) a.scan_idx_out[row] = a.scan_idx[row];
  const float *cloud = a.cloud + a.offset[scene] * C;
  const float floor = a.floor[scene];
  const unsigned key = draw_key(a.seed, a.counter, (unsigned)row, SB_DRAW_STUDENT);
  const int h = feistel_half_bits(n);
  float *out = a.point_clouds + (size_t)row * N * OC;
  for (int k = 0; k < kPerThread; ++k) {
    const int j = chunk * kChunk + k * kBlock + t;
    if (j >= N) break;
    const int p = a.idx_in ? a.idx_in[(size_t)row * N + j] : sample_index(key, j, n, N, h);
    float e[7];
    eval_row(sun, color, cloud + (size_t)p * C, floor, e);
    store_row(out + (size_t)j * OC, color, height, e);
  }
}

__global__ void __launch_bounds__(kBlock) scan_semi_kernel(const ScanSemiArgs a) {
  __shared__ RowAug s_aug;
  const int chunk = blockIdx.x, r = blockIdx.y, teacher = blockIdx.z, t = threadIdx.x;
  const int scene = a.scene[r];
  const int n = a.count[scene], N = a.N, C = a.C;
  const bool color = a.use_color != 0, height = a.use_height != 0;
  const bool sun = a.dataset == SCAN_DATASET_SUNRGBD;
  const int OC = 3 + (color ? 3 : 0) + (height ? 1 : 0);
  if (t == 0 && !teacher) {
    const RowAug g = row_aug(sun, a.u_in, r, a.seed, a.counter, (unsigned)(a.row0 + r));
    s_aug = g;
    if (chunk == 0) {  // the row's header, which the labeled builders' box kernels write
      a.supervised_mask[r] = 0;
      a.scan_idx_out[r] = a.scan_idx[r];
      write_row_header(a, r, g);
    }
  }
  __syncthreads();
  const RowAug g = teacher ? row_identity() : s_aug;
  const float *cloud = a.cloud + a.offset[scene] * C;
  const float floor = a.floor[scene];
  const int *given = teacher ? a.ema_idx_in : a.idx_in;
  const unsigned key = draw_key(a.seed, a.counter, (unsigned)(a.row0 + r),
                                teacher ? SB_DRAW_EMA : SB_DRAW_STUDENT);
  const int h = feistel_half_bits(n);
  float *out = (teacher ? a.ema_point_clouds : a.point_clouds) + (size_t)r * N * OC;
  // The kernel waits on its gathers and on little else, so a thread issues all eight before it uses
  // the first.  A slot past N reads point 0 (every scan has one) and stores nothing.
  int p[kPerThread];
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const int j = chunk * kChunk + k * kBlock + t;
    p[k] = j >= N ? 0 : (given ? given[(size_t)r * N + j] : sample_index(key, j, n, N, h));
  }
  float raw[kPerThread][6];  // constant indices only: registers, no scratch
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const float *src = cloud + (size_t)p[k] * C;
#pragma unroll
    for (int c = 0; c < 6; ++c) raw[k][c] = (c < 3 || color) ? src[c] : 0.0f;
  }
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const int j = chunk * kChunk + k * kBlock + t;
    if (j >= N) break;
    float e[7];
    eval_row(sun, color, raw[k], floor, e);
    if (sun) {  // the unlabeled dataset's / 256 in float32, on both samples
#pragma unroll
      for (int c = 3; c < 6; ++c) e[c] *= 0.00390625f;
    }
    if (!teacher) {
      aug_point(g, e[0], e[1], e[2]);
      e[6] = aug_scale(g, e[6]);
    }
    store_row(out + (size_t)j * OC, color, height, e);
  }
}

__global__ void __launch_bounds__(kBlock) scan_pack_kernel(const ScanPackArgs a) {
  __shared__ float s_key[SCAN_MAX_K];
  __shared__ int s_src[SCAN_MAX_K];
  __shared__ int s_count;
  const int b = blockIdx.x, t = threadIdx.x, K = a.K;
  const size_t in0 = (size_t)b * K, out0 = (size_t)(a.scene0 + b) * K;
  if (t == 0) s_count = 0;
  __syncthreads();
  int mine = 0;
  for (int k = t; k < K; k += kBlock) {
    const float p = a.obj_prob[in0 + k];
    const bool kept = a.keep[in0 + k] != 0 && p >= 0.0f;  // (a NaN is no detection: no rank)
    s_key[k] = kept ? p : -1.0f;  // probabilities are >= 0: never outranked
    mine += kept ? 1 : 0;
  }
  if (mine) atomicAdd(&s_count, mine);
  __syncthreads();
  const int count = s_count;
  for (int k = t; k < K; k += kBlock)
    if (s_key[k] >= 0.0f) s_src[pseudo_rank::rank(s_key, K, k)] = k;
  __syncthreads();
  if (t == 0) a.count[a.scene0 + b] = count;
  for (int r = t; r < K; r += kBlock) {
    const bool live = r < count;
    const int k = live ? s_src[r] : 0;
    a.proposal[out0 + r] = live ? k : 0;
    a.cls_out[out0 + r] = live ? (int)a.cls[in0 + k] : 0;
  }
  const int SW = a.NC > 0 ? a.NC : 1;
  for (int i = t; i < K * SW; i += kBlock) {
    const int r = i / SW, w = i - r * SW;
    a.score_out[out0 * SW + i] = r < count ? a.score[(in0 + s_src[r]) * SW + w] : 0.0f;
  }
  for (int i = t; i < K * 7; i += kBlock) {
    const int r = i / 7, w = i - r * 7;
    float x = 0.0f;
    if (r < count) {
      const size_t k = in0 + s_src[r];
      x = w < 3 ? a.center[k * 3 + w] : (w < 6 ? (float)a.size[k * 3 + (w - 3)] : (float)a.heading[k]);
    }
    a.box[out0 * 7 + i] = x;
  }
  for (int i = t; i < K * 24; i += kBlock) {
    const int r = i / 24, w = i - r * 24;
    a.corners_out[out0 * 24 + i] = r < count ? a.corners[(in0 + s_src[r]) * 24 + w] : 0.0f;
  }
}

}  // namespace

PN2_API int scene_scan_prepare(const ScanPrepareArgs *args, void *stream) {
  if (!args || args->S < 1 || (args->C != 3 && args->C != 6) || !args->cloud || !args->offset ||
      !args->count || !args->floor || !args->nonfinite)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(scan_prepare_kernel, dim3(args->S), dim3(kPrepBlock), 0, (hipStream_t)stream, *args);
  return (int)hipGetLastError();
}

PN2_API int scene_scan_batch_build(const ScanBatchArgs *args, void *stream) {
  if (!args || args->B < 1 || args->B > SB_MAX_B || args->N < 1 || (args->C != 3 && args->C != 6) ||
      (args->use_color && args->C != 6) || !args->cloud || !args->offset || !args->count ||
      !args->floor || !args->point_clouds || !args->scan_idx_out ||
      (args->dataset != SCAN_DATASET_SCANNET && args->dataset != SCAN_DATASET_SUNRGBD))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(scan_batch_kernel, dim3(pn2_ceil_div(args->N, kChunk), args->B), dim3(kBlock), 0,
                     (hipStream_t)stream, *args);
  return (int)hipGetLastError();
}

PN2_API int scene_scan_semi_build(const ScanSemiArgs *args, void *stream) {
  if (!args || args->B < 1 || args->B > SB_MAX_B || args->row0 < 0 || args->row0 + args->B > SB_MAX_B ||
      args->N < 1 || (args->C != 3 && args->C != 6) || (args->use_color && args->C != 6) ||
      (args->dataset != SCAN_DATASET_SCANNET && args->dataset != SCAN_DATASET_SUNRGBD) || !args->cloud ||
      !args->offset || !args->count || !args->floor || !args->point_clouds || !args->ema_point_clouds ||
      !args->flip_x_axis || !args->flip_y_axis || !args->rot_angle || !args->rot_mat || !args->scale ||
      !args->supervised_mask || !args->scan_idx_out)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(scan_semi_kernel, dim3(pn2_ceil_div(args->N, kChunk), args->B, 2), dim3(kBlock), 0,
                     (hipStream_t)stream, *args);
  return (int)hipGetLastError();
}

PN2_API int scene_detections_pack(const ScanPackArgs *args, void *stream) {
  if (!args || args->B < 1 || args->K < 1 || args->K > SCAN_MAX_K || args->NC < 0 || args->scene0 < 0 ||
      !args->keep || !args->obj_prob || !args->cls || !args->score || !args->center || !args->size ||
      !args->heading || !args->corners || !args->count || !args->proposal || !args->cls_out ||
      !args->score_out || !args->box || !args->corners_out)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(scan_pack_kernel, dim3(args->B), dim3(kBlock), 0, (hipStream_t)stream, *args);
  return (int)hipGetLastError();
}
