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
//                         float32, and for the student the dataset's flip / rotate / scale RESTATED
//                         from scene_points_kernel / sun_points_kernel (float64 per stage, rounded to
//                         float32 after each; the parity tests hold the copies equal).  All eight
//                         gathers of a thread are issued before the first is used.  One thread per
//                         row writes the header scene_boxes_kernel / sun_boxes_kernel write.
//   scan_pack_kernel      one workgroup per scene: the kept proposals ranked by (objectness
//                         probability descending, proposal ascending) with pseudo_rank::rank, then
//                         every plane of the scene's arena rows written in row order -- rows past
//                         the count as zeros, so the arena needs no clear.
#include "common.h"
#include "scene_common.h"
#include "pseudo_rank.h"
#include "../../include/scan_hip.h"
#include "../../include/sunrgbd_hip.h"  // SUN_DRAW_FLIP

namespace {

constexpr int kPrepBlock = 1024;
constexpr int kPrepWaves = kPrepBlock / kWave;
constexpr int kBlock = 256;
constexpr int kPerThread = 8;
constexpr int kChunk = kBlock * kPerThread;  // sample slots per workgroup of scan_batch_kernel

__device__ __forceinline__ unsigned order_key(float f) {  // monotone: a < b <=> key(a) < key(b)
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float from_order_key(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

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

__global__ void __launch_bounds__(kBlock) scan_batch_kernel(const ScanBatchArgs a) {
  const int chunk = blockIdx.x, row = blockIdx.y, t = threadIdx.x;
  const int scene = a.scene[row];
  const int n = a.count[scene], N = a.N, C = a.C;
  const int OC = 3 + (a.use_color ? 3 : 0) + (a.use_height ? 1 : 0);
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
    const float *src = cloud + (size_t)p * C;
    float *dst = out + (size_t)j * OC;
    const float z = src[2];
    dst[0] = src[0];
    dst[1] = src[1];
    dst[2] = z;
    int c = 3;
    if (a.use_color) {
      if (a.dataset == SCAN_DATASET_SCANNET) {  // (rgb - MEAN_COLOR_RGB) / 256.0
        dst[3] = (float)(((double)src[3] - 109.8) / 256.0);
        dst[4] = (float)(((double)src[4] - 97.2) / 256.0);
        dst[5] = (float)(((double)src[5] - 83.8) / 256.0);
      } else {  // rgb - MEAN_COLOR_RGB, 0.5 each
        dst[3] = (float)((double)src[3] - 0.5);
        dst[4] = (float)((double)src[4] - 0.5);
        dst[5] = (float)((double)src[5] - 0.5);
      }
      c = 6;
    }
    if (a.use_height) dst[c] = __fsub_rn(z, floor);
  }
}

struct SemiAug {
  int fx, fy;
  double c, s, angle, scale;
};

__device__ __forceinline__ double semi_uniform(const ScanSemiArgs &a, int r, int k) {
  const bool sun = a.dataset == SCAN_DATASET_SUNRGBD;
  if (a.u_in) return a.u_in[r * (sun ? 3 : 4) + k];
  const unsigned first = sun ? (unsigned)SUN_DRAW_FLIP : (unsigned)SB_DRAW_FLIP_X;
  return (double)draw_key(a.seed, a.counter, (unsigned)(a.row0 + r), first + k) * 0x1p-32;
}

// row_aug of scene_batch.hip and sun_row_aug of sunrgbd_batch.hip, restated
__device__ __forceinline__ SemiAug semi_row_aug(const ScanSemiArgs &a, int r) {
  SemiAug g;
  g.fx = semi_uniform(a, r, 0) > 0.5;
  if (a.dataset == SCAN_DATASET_SUNRGBD) {
    g.fy = 0;
    g.angle = (semi_uniform(a, r, 1) * M_PI) / 3.0 - M_PI / 6.0;  // -30 ~ +30 degree
    g.scale = semi_uniform(a, r, 2) * 0.3 + 0.85;
  } else {
    g.fy = semi_uniform(a, r, 1) > 0.5;
    g.angle = (semi_uniform(a, r, 2) * M_PI) / 18.0 - M_PI / 36.0;  // -5 ~ +5 degree
    g.scale = semi_uniform(a, r, 3) * 0.3 + 0.85;
  }
  g.c = cos(g.angle);
  g.s = sin(g.angle);
  return g;
}

__global__ void __launch_bounds__(kBlock) scan_semi_kernel(const ScanSemiArgs a) {
  __shared__ SemiAug s_aug;
  const int chunk = blockIdx.x, r = blockIdx.y, teacher = blockIdx.z, t = threadIdx.x;
  const int scene = a.scene[r];
  const int n = a.count[scene], N = a.N, C = a.C;
  const bool color = a.use_color != 0, height = a.use_height != 0;
  const bool sun = a.dataset == SCAN_DATASET_SUNRGBD;
  const int OC = 3 + (color ? 3 : 0) + (height ? 1 : 0);
  if (t == 0 && !teacher) {
    const SemiAug g = semi_row_aug(a, r);
    s_aug = g;
    if (chunk == 0) {  // the row's header, as the labeled builders' box kernels write it
      a.supervised_mask[r] = 0;
      a.scan_idx_out[r] = a.scan_idx[r];
      a.flip_x_axis[r] = g.fx;
      a.flip_y_axis[r] = g.fy;
      a.rot_angle[r] = (float)g.angle;
      float *m = a.rot_mat + r * 9;
      m[0] = (float)g.c; m[1] = (float)-g.s; m[2] = 0.0f;
      m[3] = (float)g.s; m[4] = (float)g.c;  m[5] = 0.0f;
      m[6] = 0.0f;       m[7] = 0.0f;        m[8] = 1.0f;
      const float sc = (float)g.scale;
      a.scale[r * 3 + 0] = sc;
      a.scale[r * 3 + 1] = sc;
      a.scale[r * 3 + 2] = sc;
    }
  }
  __syncthreads();
  SemiAug g{};
  if (!teacher) g = s_aug;
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
    float x = raw[k][0], y = raw[k][1], z = raw[k][2];
    float rgb[3] = {0.0f, 0.0f, 0.0f};
    if (color) {
      if (sun) {  // rgb - MEAN_COLOR_RGB, 0.5 each, then the unlabeled dataset's / 256 in float32
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb[c] = (float)((double)raw[k][3 + c] - 0.5) * 0.00390625f;
      } else {  // (rgb - MEAN_COLOR_RGB) / 256.0
        rgb[0] = (float)(((double)raw[k][3] - 109.8) / 256.0);
        rgb[1] = (float)(((double)raw[k][4] - 97.2) / 256.0);
        rgb[2] = (float)(((double)raw[k][5] - 83.8) / 256.0);
      }
    }
    float up = __fsub_rn(z, floor);
    if (!teacher) {
      if (g.fx) x = -x;
      if (g.fy) y = -y;
      const double dx = x, dy = y, dz = z;
      const float rx = (float)(dx * g.c + dy * -g.s + dz * 0.0);
      const float ry = (float)(dx * g.s + dy * g.c + dz * 0.0);
      const float rz = (float)(dx * 0.0 + dy * 0.0 + dz * 1.0);
      x = (float)((double)rx * g.scale);
      y = (float)((double)ry * g.scale);
      z = (float)((double)rz * g.scale);
      up = (float)((double)up * g.scale);
    }
    float *dst = out + (size_t)j * OC;
    dst[0] = x;
    dst[1] = y;
    dst[2] = z;
    if (color) {
      dst[3] = rgb[0];
      dst[4] = rgb[1];
      dst[5] = rgb[2];
    }
    if (height) dst[OC - 1] = up;
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
