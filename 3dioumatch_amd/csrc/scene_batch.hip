// 3dioumatch_amd/csrc/scene_batch.hip -- ScanNet train / eval batches built on the device from the
// resident scene store (include/scene_hip.h; votenet/scannet_data.py is the host restatement).
//
// Three launches per batch, all small grids (they run beside the train step on its side stream):
//   scene_boxes_kernel    one workgroup per row: the row's draws (flip x / flip y / angle / scale ->
//                         flip_x_axis, flip_y_axis, rot_angle, rot_mat, scale), its box labels
//                         (flip, rotate_aligned_boxes, scale in float64 as model_util_scannet.py:
//                         85-106 does), scan_idx / supervised_mask, and -- for a vote row -- the
//                         clear of its instance table.
//   scene_points_kernel   (chunks of 2048 sample slots) x rows x (student, teacher): the sample
//                         index of each slot (keyed Feistel bijection + cycle walking when the
//                         scene has >= N points, i.i.d. draws otherwise), the gathered row, the
//                         student's augmentation (float64, rounded to float32 after each stage as
//                         the reference's float32 cloud is), and for vote rows the per-instance
//                         extents of the chunk: order-preserving integer keys min / max'ed in an
//                         LDS table (7 words per instance), merged into the row's global table
//                         with one set of integer atomics per instance the chunk touched.
//   scene_votes_kernel    one lane per (vote row, slot): 0.5 (min + max) - x of its instance, masked
//                         by the semantic label at the instance's FIRST sampled position
//                         (scannet_ssl_dataset.py:136-147).  Integer atomics make the result
//                         independent of arrival order: bit-reproducible.
// The draws, the row header, the point's and the box centre's flip / rotate / scale and the integer
// keys are csrc/scene_common.h's (row_aug, write_row_header, aug_point, aug_vector, order_key), which
// the other two builders call too; what is written out here is ScanNet's own: the extent rule of
// rotate_aligned_boxes, the instance tables and the votes.
#include "common.h"
#include "scene_common.h"
#include "../../include/scene_hip.h"

namespace {

constexpr int kBlock = 256;
constexpr int kPerThread = 8;
constexpr int kChunk = kBlock * kPerThread;  // sample slots per workgroup of scene_points_kernel
constexpr int kTableWords = 8;               // minx miny minz maxx maxy maxz first pad

__constant__ int kNyu40ids[18] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39};

__device__ __forceinline__ bool is_nyu40(int id) {
  bool hit = false;
#pragma unroll
  for (int i = 0; i < 18; ++i) hit |= kNyu40ids[i] == id;
  return hit;
}

__global__ void __launch_bounds__(kBlock) scene_boxes_kernel(const SceneBatchArgs a) {
  const int row = blockIdx.x, t = threadIdx.x;
  const int scene = a.scene[row];
  const bool train = a.augment != 0;
  const RowAug g = train ? row_aug(false, a.u_in, row, a.seed, a.counter, (unsigned)row) : row_identity();
  if (t == 0) {
    if (a.supervised_mask) a.supervised_mask[row] = a.supervised[row];
    if (a.scan_idx_out) a.scan_idx_out[row] = a.scan_idx[row];
    write_row_header(a, row, g);
  }
  if (row < a.vote_rows) {  // the instance table the points kernel fills
    const int words = a.ninst[scene] * kTableWords;
    unsigned *tab = a.table + (size_t)row * SB_MAX_INST * kTableWords;
    for (int i = t; i < words; i += kBlock) {
      const int w = i % kTableWords;
      tab[i] = (w < 3 || w == 6) ? 0xFFFFFFFFu : 0u;
    }
  }
  if (row >= a.box_rows || t >= SB_MAX_OBJ) return;
  const int nb = a.nbox[scene];
  const double *src = a.boxes + ((size_t)scene * SB_MAX_OBJ + t) * SB_BOX_COLS;
  double cx = 0.0, cy = 0.0, cz = 0.0, dx = 0.0, dy = 0.0, dz = 0.0;
  int cls = 0;
  if (t < nb) {
    cx = src[0]; cy = src[1]; cz = src[2]; dx = src[3]; dy = src[4]; dz = src[5];
    cls = (int)src[6];
  }
  if (train && row < a.box_aug_rows) {
    // rotate_aligned_boxes: centres by rot_mat, x/y extent = 2 x the largest rotated half-corner
    aug_vector(g, cx, cy, cz);
    const double c = g.c, s = g.s;
    const double hx = dx / 2.0, hy = dy / 2.0;
    double mx = -INFINITY, my = -INFINITY;
    const double sx[4] = {-1.0, 1.0, 1.0, -1.0}, sy[4] = {-1.0, -1.0, 1.0, 1.0};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double px = sx[k] * hx, py = sy[k] * hy;
      mx = fmax(mx, px * c + py * -s + 0.0 * 0.0);
      my = fmax(my, px * s + py * c + 0.0 * 0.0);
    }
    dx = (2.0 * mx) * g.scale; dy = (2.0 * my) * g.scale; dz = dz * g.scale;
  }
  const size_t o = (size_t)row * SB_MAX_OBJ + t;
  a.center_label[o * 3 + 0] = (float)cx;
  a.center_label[o * 3 + 1] = (float)cy;
  a.center_label[o * 3 + 2] = (float)cz;
  a.heading_class_label[o] = 0;
  a.heading_residual_label[o] = 0.0f;
  a.size_class_label[o] = t < nb ? cls : 0;
  a.sem_cls_label[o] = t < nb ? cls : 0;
  a.box_label_mask[o] = t < nb ? 1.0f : 0.0f;
  const double *mean = a.mean_size + 3 * (t < nb ? cls : 0);
  a.size_residual_label[o * 3 + 0] = t < nb ? (float)(dx - mean[0]) : 0.0f;
  a.size_residual_label[o * 3 + 1] = t < nb ? (float)(dy - mean[1]) : 0.0f;
  a.size_residual_label[o * 3 + 2] = t < nb ? (float)(dz - mean[2]) : 0.0f;
}

__global__ void __launch_bounds__(kBlock) scene_points_kernel(const SceneBatchArgs a) {
  __shared__ unsigned s_tab[7 * SB_MAX_INST];
  __shared__ RowAug s_aug;
  const int chunk = blockIdx.x, row = blockIdx.y, teacher = blockIdx.z, t = threadIdx.x;
  const int scene = a.scene[row];
  const int n = a.count[scene], N = a.N, C = a.C;
  const bool augment = !teacher && a.augment;
  const bool votes = !teacher && row < a.vote_rows;
  const int ninst = votes ? a.ninst[scene] : 0;
  if (t == 0 && augment) s_aug = row_aug(false, a.u_in, row, a.seed, a.counter, (unsigned)row);
  for (int i = t; i < 7 * ninst; i += kBlock) s_tab[i] = (i < 3 * ninst || i >= 6 * ninst) ? 0xFFFFFFFFu : 0u;
  __syncthreads();
  const RowAug g = augment ? s_aug : row_identity();
  const float *cloud = a.cloud + a.offset[scene] * C;
  const int *given = teacher ? a.ema_idx_in : a.idx_in;
  const unsigned key = draw_key(a.seed, a.counter, (unsigned)row, teacher ? SB_DRAW_EMA : SB_DRAW_STUDENT);
  const int h = feistel_half_bits(n);
  float *out = (teacher ? a.ema_point_clouds : a.point_clouds) + (size_t)row * N * C;
  for (int k = 0; k < kPerThread; ++k) {
    const int j = chunk * kChunk + k * kBlock + t;
    if (j >= N) break;
    const int p = given ? given[(size_t)row * N + j] : sample_index(key, j, n, N, h);
    const float *src = cloud + (size_t)p * C;
    float v[7];  // channels 3..6 only ever move as a whole: constant indices, no scratch
#pragma unroll
    for (int c = 0; c < 7; ++c) v[c] = c < C ? src[c] : 0.0f;
    if (augment) {
      aug_point(g, v[0], v[1], v[2]);
#pragma unroll
      for (int c = 3; c < 7; ++c)
        if (a.has_height && c == C - 1) v[c] = aug_scale(g, v[c]);
    }
#pragma unroll
    for (int c = 0; c < 7; ++c)
      if (c < C) out[(size_t)j * C + c] = v[c];
    if (votes) {
      a.idx_out[(size_t)row * N + j] = p;
      const int i = a.inst[a.offset[scene] + p];
      for (int c = 0; c < 3; ++c) {
        atomicMin(&s_tab[c * ninst + i], order_key(v[c]));
        atomicMax(&s_tab[(3 + c) * ninst + i], order_key(v[c]));
      }
      atomicMin(&s_tab[6 * ninst + i], (unsigned)j);
    }
  }
  if (!votes) return;
  __syncthreads();
  unsigned *tab = a.table + (size_t)row * SB_MAX_INST * kTableWords;
  for (int i = t; i < ninst; i += kBlock) {
    if (s_tab[6 * ninst + i] == 0xFFFFFFFFu) continue;  // not in this chunk
    unsigned *e = tab + (size_t)i * kTableWords;
    for (int c = 0; c < 3; ++c) {
      atomicMin(&e[c], s_tab[c * ninst + i]);
      atomicMax(&e[3 + c], s_tab[(3 + c) * ninst + i]);
    }
    atomicMin(&e[6], s_tab[6 * ninst + i]);
  }
}

__global__ void __launch_bounds__(kBlock) scene_votes_kernel(const SceneBatchArgs a) {
  const int row = blockIdx.y, j = blockIdx.x * kBlock + threadIdx.x;
  const int N = a.N, C = a.C;
  if (j >= N) return;
  const int scene = a.scene[row];
  const long long off = a.offset[scene];
  const int *idx = a.idx_out + (size_t)row * N;
  const int i = a.inst[off + idx[j]];
  const unsigned *e = a.table + ((size_t)row * SB_MAX_INST + i) * kTableWords;
  const bool hit = is_nyu40(a.sem[off + idx[e[6]]]);
  const float *pt = a.point_clouds + ((size_t)row * N + j) * C;
  float vote[3];
  for (int c = 0; c < 3; ++c) {
    const float centre = 0.5f * (from_order_key(e[c]) + from_order_key(e[3 + c]));
    vote[c] = hit ? centre - pt[c] : 0.0f;
  }
  float *dst = a.vote_label + ((size_t)row * N + j) * 9;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) dst[r * 3 + c] = vote[c];
  a.vote_label_mask[(size_t)row * N + j] = hit ? 1 : 0;
}

bool valid(const SceneBatchArgs *a) {
  if (!a || a->B < 1 || a->B > SB_MAX_B || a->N < 1 || a->C < 3 || a->C > 7) return false;
  if (a->vote_rows < 0 || a->vote_rows > a->B || a->box_rows < 0 || a->box_rows > a->B) return false;
  if (a->box_aug_rows < 0 || a->box_aug_rows > a->box_rows) return false;
  if (!a->cloud || !a->inst || !a->sem || !a->offset || !a->count || !a->ninst || !a->point_clouds)
    return false;
  if (a->ema && !a->ema_point_clouds) return false;
  if (a->vote_rows && (!a->idx_out || !a->table || !a->vote_label || !a->vote_label_mask))
    return false;
  if (a->box_rows && (!a->boxes || !a->nbox || !a->mean_size || !a->center_label ||
                      !a->heading_class_label || !a->heading_residual_label ||
                      !a->size_class_label || !a->size_residual_label || !a->sem_cls_label ||
                      !a->box_label_mask))
    return false;
  if (a->flip_x_axis && (!a->flip_y_axis || !a->rot_angle || !a->rot_mat || !a->scale)) return false;
  return true;
}

}  // namespace

PN2_API int scene_batch_build(const SceneBatchArgs *args, void *stream) {
  if (!valid(args)) return (int)hipErrorInvalidValue;
  const hipStream_t s = (hipStream_t)stream;
  const SceneBatchArgs &a = *args;
  hipLaunchKernelGGL(scene_boxes_kernel, dim3(a.B), dim3(kBlock), 0, s, a);
  hipLaunchKernelGGL(scene_points_kernel, dim3(pn2_ceil_div(a.N, kChunk), a.B, a.ema ? 2 : 1),
                     dim3(kBlock), 0, s, a);
  if (a.vote_rows > 0)
    hipLaunchKernelGGL(scene_votes_kernel, dim3(pn2_ceil_div(a.N, kBlock), a.vote_rows),
                       dim3(kBlock), 0, s, a);
  return (int)hipGetLastError();
}
