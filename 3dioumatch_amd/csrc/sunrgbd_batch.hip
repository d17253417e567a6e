// 3dioumatch_amd/csrc/sunrgbd_batch.hip -- SUN RGB-D train / eval batches built on the device from
// the resident scene store (include/sunrgbd_hip.h; votenet/sunrgbd_data.py is the host restatement).
//
// Two launches per batch, both small grids (they run beside the train step on its side stream):
//   sun_boxes_kernel    one 64-lane workgroup per row, one lane per box slot: the row's draws
//                       (flip / angle / scale -> flip_x_axis, flip_y_axis = 0, rot_angle, rot_mat,
//                       scale), its oriented-box labels in float64 in the reference's operation
//                       order (sunrgbd_detection_dataset.py:155-226: centre flip / rotate / scale,
//                       heading pi - theta, theta - rot_angle, angle2class with Python's float
//                       modulo, size residual of 2 x the half size against the class's mean size),
//                       masks, scan_idx and supervised_mask.
//   sun_points_kernel   (chunks of 2048 sample slots) x rows x (student, teacher): the sample index
//                       of each slot, the gathered cloud row, the unlabeled rows' colour / 256, the
//                       detection dataset's colour augmentation (per-point draws keyed by the
//                       SOURCE index, so only sampled points are computed), flip / rotate / scale
//                       rounded to float32 after each stage as the reference's float32 cloud is,
//                       and on vote rows the gathered (mask, 3 votes) row carried through the same
//                       flip, rotation and scale.  rot(p + v) - rot(p) is computed as rot(v): the
//                       two differ by the float32 rounding of the rotated point only.  For a
//                       store without vote rows (votes == NULL) the <true> instantiation computes
//                       the row from the SOURCE point and the scene's boxes instead of loading it.
// One launch for the whole store (scene_sunrgbd_votes), for inspection and export:
//   sun_votes_kernel    (point chunks, grid-strided) x scenes: the (mask, 3 votes) row of every
//                       stored point in the reference's layout.
// The vote rule (sunrgbd/sunrgbd_data.py:232-257 with the hull of sunrgbd_utils.py:227-237, which
// is the oriented box itself) is sun_vote_row, shared by the two kernels: the scene's boxes staged
// once per workgroup in LDS (64 x 8 doubles), every test in float64, the slot picked by selects.
// No atomics, no scratch tables: a slot's outputs depend on its own source row alone.
// The draws, the row header, the point's flip / rotate / scale and the float64 one of the box centres
// and the votes are csrc/scene_common.h's (row_aug, write_row_header, aug_point, aug_vector), which
// the other two builders call too; what is written out here is SUN RGB-D's own: heading and half
// sizes, the colour augmentation and the vote rule.
#include "common.h"
#include "scene_common.h"
#include "../../include/sunrgbd_hip.h"

namespace {

constexpr int kBlock = 256;
constexpr int kPerThread = 8;
constexpr int kChunk = kBlock * kPerThread;  // sample slots per workgroup of sun_points_kernel

// Python's float modulo for a positive divisor: the result takes the divisor's sign
__device__ __forceinline__ double py_mod(double x, double y) {
  double m = fmod(x, y);
  if (m != 0.0) {
    if (m < 0.0) m += y;
  } else {
    m = 0.0;
  }
  return m;
}

__global__ void __launch_bounds__(SUN_MAX_OBJ) sun_boxes_kernel(const SunBatchArgs a) {
  const int row = blockIdx.x, t = threadIdx.x;
  const int scene = a.scene[row];
  const bool train = a.augment != 0;
  const RowAug g = train ? row_aug(true, a.u_in, row, a.seed, a.counter, (unsigned)row) : row_identity();
  if (t == 0) {
    if (a.supervised_mask) a.supervised_mask[row] = a.supervised[row];
    if (a.scan_idx_out) a.scan_idx_out[row] = a.scan_idx[row];
    write_row_header(a, row, g);
  }
  if (row >= a.box_rows) return;
  const int nb = a.nbox[scene];
  const bool live = t < nb;
  const double *src = a.boxes + ((size_t)scene * SUN_MAX_OBJ + t) * SUN_BOX_COLS;
  double cx = 0.0, cy = 0.0, cz = 0.0, hx = 0.0, hy = 0.0, hz = 0.0, heading = 0.0;
  int cls = 0;
  if (live) {
    cx = src[0]; cy = src[1]; cz = src[2]; hx = src[3]; hy = src[4]; hz = src[5];
    heading = src[6];
    cls = (int)src[7];
  }
  if (train && row < a.box_aug_rows) {
    aug_vector(g, cx, cy, cz);
    if (g.fx) heading = M_PI - heading;
    heading -= g.angle;
    hx = hx * g.scale; hy = hy * g.scale; hz = hz * g.scale;
  }
  // angle2class (model_util_sunrgbd.py:92-108)
  const double two_pi = 2.0 * M_PI;
  const double per = two_pi / (double)a.num_heading_bin;
  const double shifted = py_mod(py_mod(heading, two_pi) + per / 2.0, two_pi);
  const int head_cls = (int)(shifted / per);
  const double head_res = shifted - ((double)head_cls * per + per / 2.0);
  const size_t o = (size_t)row * SUN_MAX_OBJ + t;
  a.center_label[o * 3 + 0] = (float)cx;
  a.center_label[o * 3 + 1] = (float)cy;
  a.center_label[o * 3 + 2] = (float)cz;
  a.heading_class_label[o] = live ? head_cls : 0;
  a.heading_residual_label[o] = live ? (float)head_res : 0.0f;
  a.size_class_label[o] = live ? cls : 0;
  a.sem_cls_label[o] = live ? cls : 0;
  a.box_label_mask[o] = live ? 1.0f : 0.0f;
  const double *mean = a.mean_size + 3 * (live ? cls : 0);
  a.size_residual_label[o * 3 + 0] = live ? (float)(hx * 2.0 - mean[0]) : 0.0f;
  a.size_residual_label[o * 3 + 1] = live ? (float)(hy * 2.0 - mean[1]) : 0.0f;
  a.size_residual_label[o * 3 + 2] = live ? (float)(hz * 2.0 - mean[2]) : 0.0f;
}

struct SunColor {
  double bright[3], shift[3];
};

// one staged box of the vote rule: centre, |half sizes|, cos / sin of the heading
struct SunBox {
  double cx, cy, cz, hx, hy, hz, c, s;
};

// Stage the scene's first `nb` (<= SUN_MAX_OBJ) box rows; the caller synchronises.  The hull of a
// box with a zero half size is flat: the reference's hull call raises and the object is skipped
// (sunrgbd_data.py:258-259), so such a box gets negative half sizes, which no point satisfies.
__device__ __forceinline__ void sun_stage_boxes(SunBox *s_box, const double *boxes, int scene, int nb,
                                                int t) {
  for (int k = t; k < nb; k += kBlock) {
    const double *src = boxes + ((size_t)scene * SUN_MAX_OBJ + k) * SUN_BOX_COLS;
    SunBox b;
    b.cx = src[0]; b.cy = src[1]; b.cz = src[2];
    b.hx = fabs(src[3]); b.hy = fabs(src[4]); b.hz = fabs(src[5]);
    if (b.hx == 0.0 || b.hy == 0.0 || b.hz == 0.0) b.hx = b.hy = b.hz = -1.0;
    b.c = cos(src[6]);
    b.s = sin(src[6]);
    s_box[k] = b;
  }
}

// The vote row of one point in the stored packing (mask x1 | y1 z1 | x2 y2 | z2 x3 | y3 z3): the
// first containing box in table order sets the mask and all three slots, the second slot 1, the
// third and every later one slot 2 (point_vote_idx saturates at 2, so the LAST one stays there).
// The loop keeps the three slots' BOX INDICES, chosen by selects on the hit count (never by
// indexing a register array); the votes are formed once after it.  `nb` is uniform in the
// workgroup and every lane reads the same LDS address inside the loop.
__device__ __forceinline__ void sun_vote_row(const SunBox *s_box, int nb, float px, float py, float pz,
                                             float2 (&w)[5]) {
  const double x = (double)px, y = (double)py, z = (double)pz;
  int k1 = 0, k2 = 0, k3 = 0, hits = 0;
  for (int k = 0; k < nb; ++k) {
    const SunBox b = s_box[k];
    const double dx = x - b.cx, dy = y - b.cy, dz = z - b.cz;
    const double lx = dx * b.c - dy * b.s;
    const double ly = dx * b.s + dy * b.c;
    const bool in = fabs(lx) <= b.hx && fabs(ly) <= b.hy && fabs(dz) <= b.hz;
    k1 = in && hits == 0 ? k : k1;
    k2 = in && hits <= 1 ? k : k2;
    k3 = in && hits != 1 ? k : k3;
    hits += in ? 1 : 0;
  }
  float v[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};  // constant indices only
  if (hits) {  // centre - point, as the reference forms it
    const int ks[3] = {k1, k2, k3};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const SunBox *b = s_box + ks[q];
      v[q * 3 + 0] = (float)(b->cx - x);
      v[q * 3 + 1] = (float)(b->cy - y);
      v[q * 3 + 2] = (float)(b->cz - z);
    }
  }
  w[0] = make_float2(hits ? 1.0f : 0.0f, v[0]);
  w[1] = make_float2(v[1], v[2]);
  w[2] = make_float2(v[3], v[4]);
  w[3] = make_float2(v[5], v[6]);
  w[4] = make_float2(v[7], v[8]);
}

__device__ __forceinline__ double sun_color_uniform(const SunBatchArgs &a, int row, int k) {
  if (a.u_color_in) return a.u_color_in[row * 6 + k];
  return (double)draw_key(a.seed, a.counter, (unsigned)row, SUN_DRAW_COLOR + k) * 0x1p-32;
}

// kFromBoxes: the store holds no vote rows (a.votes == NULL); they are computed from the boxes
template <bool kFromBoxes>
__global__ void __launch_bounds__(kBlock) sun_points_kernel(const SunBatchArgs a) {
  __shared__ RowAug s_aug;
  __shared__ SunColor s_col;
  __shared__ SunBox s_box[kFromBoxes ? SUN_MAX_OBJ : 1];
  const int chunk = blockIdx.x, row = blockIdx.y, teacher = blockIdx.z, t = threadIdx.x;
  const int scene = a.scene[row];
  const int n = a.count[scene], N = a.N, C = a.C;
  const bool augment = !teacher && a.augment;
  const bool votes = !teacher && row < a.vote_rows;
  const bool color = augment && a.color_aug && C >= 6;
  const bool div256 = row >= a.div256_from && C >= 6;
  if (t == 0 && augment) s_aug = row_aug(true, a.u_in, row, a.seed, a.counter, (unsigned)row);
  if (t < 3 && color) {
    s_col.bright[t] = 1.0 + 0.4 * sun_color_uniform(a, row, t) - 0.2;
    s_col.shift[t] = 0.1 * sun_color_uniform(a, row, 3 + t) - 0.05;
  }
  int nb = 0;
  if constexpr (kFromBoxes) {
    if (votes) {
      nb = min(a.nbox[scene], SUN_MAX_OBJ);
      sun_stage_boxes(s_box, a.boxes, scene, nb, t);
    }
  }
  __syncthreads();
  const RowAug g = augment ? s_aug : row_identity();
  SunColor col{};
  if (color) col = s_col;
  const long long off = a.offset[scene];
  const float *cloud = a.cloud + off * C;
  const float *vrow = a.votes + off * SUN_VOTE_COLS;
  const int *given = teacher ? a.ema_idx_in : a.idx_in;
  const unsigned key = draw_key(a.seed, a.counter, (unsigned)row, teacher ? SUN_DRAW_EMA : SUN_DRAW_STUDENT);
  const unsigned key_jit = draw_key(a.seed, a.counter, (unsigned)row, SUN_DRAW_JITTER);
  const unsigned key_drop = draw_key(a.seed, a.counter, (unsigned)row, SUN_DRAW_DROP);
  const double *u_point = a.u_point_in ? a.u_point_in + (size_t)row * 2 * a.u_point_stride : nullptr;
  const int h = feistel_half_bits(n);
  float *out = (teacher ? a.ema_point_clouds : a.point_clouds) + (size_t)row * N * C;
  for (int k = 0; k < kPerThread; ++k) {
    const int j = chunk * kChunk + k * kBlock + t;
    if (j >= N) break;
    const int p = given ? given[(size_t)row * N + j] : sample_index(key, j, n, N, h);
    const float *src = cloud + (size_t)p * C;
    float v[7];  // constant indices only: registers, no scratch
#pragma unroll
    for (int c = 0; c < 7; ++c) v[c] = c < C ? src[c] : 0.0f;
    float2 w[5];  // mask x1 | y1 z1 | x2 y2 | z2 x3 | y3 z3 (rows are 8-byte aligned)
    if (votes) {
      if constexpr (kFromBoxes) {
        sun_vote_row(s_box, nb, v[0], v[1], v[2], w);
      } else {
        const float2 *vs = reinterpret_cast<const float2 *>(vrow + (size_t)p * SUN_VOTE_COLS);
#pragma unroll
        for (int q = 0; q < 5; ++q) w[q] = vs[q];
      }
    }
    if (div256) {
      v[3] *= 0.00390625f;
      v[4] *= 0.00390625f;
      v[5] *= 0.00390625f;
    }
    if (augment) {
      aug_point(g, v[0], v[1], v[2]);
      if (color) {  // (touches channels 3..5 only; the height channel is scaled after it)
        const double uj = u_point ? u_point[p] : (double)element(key_jit, (unsigned)p) * 0x1p-32;
        const double ud = u_point ? u_point[a.u_point_stride + p]
                                  : (double)element(key_drop, (unsigned)p) * 0x1p-32;
        const double jitter = 0.05 * uj - 0.025;
        const double keep = ud > 0.3 ? 1.0 : 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          double rgb = (double)v[3 + c] + 0.5;
          rgb = rgb * col.bright[c];
          rgb = rgb + col.shift[c];
          rgb = rgb + jitter;
          rgb = fmin(fmax(rgb, 0.0), 1.0);
          rgb = rgb * keep;
          v[3 + c] = (float)(rgb - 0.5);
        }
      }
#pragma unroll
      for (int c = 3; c < 7; ++c)
        if (a.has_height && c == C - 1) v[c] = aug_scale(g, v[c]);
    }
#pragma unroll
    for (int c = 0; c < 7; ++c)
      if (c < C) out[(size_t)j * C + c] = v[c];
    if (votes) {
      const float vx[3] = {w[0].y, w[2].x, w[3].y};
      const float vy[3] = {w[1].x, w[2].y, w[4].x};
      const float vz[3] = {w[1].y, w[3].x, w[4].y};
      float *dst = a.vote_label + ((size_t)row * N + j) * 9;
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        double x = vx[q], y = vy[q], z = vz[q];
        if (augment) aug_vector(g, x, y, z);
        dst[q * 3 + 0] = (float)x;
        dst[q * 3 + 1] = (float)y;
        dst[q * 3 + 2] = (float)z;
      }
      a.vote_label_mask[(size_t)row * N + j] = (long long)w[0].x;
    }
  }
}

constexpr int kVoteChunks = 32;  // grid.x of sun_votes_kernel: a 50k-point scan is 25 chunks

__global__ void __launch_bounds__(kBlock) sun_votes_kernel(const float *cloud, int C,
                                                           const long long *offset, const int *count,
                                                           const double *boxes, const int *nbox,
                                                           float *votes_out) {
  __shared__ SunBox s_box[SUN_MAX_OBJ];
  const int scene = blockIdx.y, t = threadIdx.x;
  const int n = count[scene];
  const int nb = min(nbox[scene], SUN_MAX_OBJ);
  sun_stage_boxes(s_box, boxes, scene, nb, t);
  __syncthreads();
  const long long off = offset[scene];
  for (long long base = (long long)blockIdx.x * kChunk; base < n; base += (long long)gridDim.x * kChunk) {
    for (int k = 0; k < kPerThread; ++k) {
      const long long j = base + k * kBlock + t;
      if (j >= n) break;
      const float *src = cloud + (size_t)(off + j) * C;
      float2 w[5];
      sun_vote_row(s_box, nb, src[0], src[1], src[2], w);
      float2 *dst = reinterpret_cast<float2 *>(votes_out + (size_t)(off + j) * SUN_VOTE_COLS);
#pragma unroll
      for (int q = 0; q < 5; ++q) dst[q] = w[q];
    }
  }
}

bool valid(const SunBatchArgs *a) {
  if (!a || a->B < 1 || a->B > SUN_MAX_B || a->N < 1 || a->C < 3 || a->C > 7) return false;
  if (a->vote_rows < 0 || a->vote_rows > a->B || a->box_rows < 0 || a->box_rows > a->B) return false;
  if (a->box_aug_rows < 0 || a->box_aug_rows > a->box_rows) return false;
  if (a->div256_from < 0 || a->num_heading_bin < 1) return false;
  if (!a->cloud || !a->offset || !a->count || !a->point_clouds) return false;
  if (a->ema && !a->ema_point_clouds) return false;
  if (a->color_aug && a->C < 6) return false;
  if (a->u_point_in && a->u_point_stride < 1) return false;
  if (a->vote_rows && (!a->vote_label || !a->vote_label_mask)) return false;
  if (a->vote_rows && !a->votes && (!a->boxes || !a->nbox)) return false;  // votes from the boxes
  if (a->box_rows && (!a->boxes || !a->nbox || !a->mean_size || !a->center_label ||
                      !a->heading_class_label || !a->heading_residual_label ||
                      !a->size_class_label || !a->size_residual_label || !a->sem_cls_label ||
                      !a->box_label_mask))
    return false;
  if (a->flip_x_axis && (!a->flip_y_axis || !a->rot_angle || !a->rot_mat || !a->scale)) return false;
  return true;
}

}  // namespace

PN2_API int scene_sunrgbd_batch_build(const SunBatchArgs *args, void *stream) {
  if (!valid(args)) return (int)hipErrorInvalidValue;
  const hipStream_t s = (hipStream_t)stream;
  const SunBatchArgs &a = *args;
  hipLaunchKernelGGL(sun_boxes_kernel, dim3(a.B), dim3(SUN_MAX_OBJ), 0, s, a);
  const dim3 grid(pn2_ceil_div(a.N, kChunk), a.B, a.ema ? 2 : 1);
  if (a.vote_rows && !a.votes)
    hipLaunchKernelGGL(sun_points_kernel<true>, grid, dim3(kBlock), 0, s, a);
  else
    hipLaunchKernelGGL(sun_points_kernel<false>, grid, dim3(kBlock), 0, s, a);
  return (int)hipGetLastError();
}

PN2_API int scene_sunrgbd_votes(const float *cloud, int C, const long long *offset, const int *count,
                                const double *boxes, const int *nbox, int scenes, float *votes_out,
                                void *stream) {
  if (!cloud || !offset || !count || !boxes || !nbox || !votes_out || C < 3 || scenes < 1 || scenes > 65535)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(sun_votes_kernel, dim3(kVoteChunks, scenes), dim3(kBlock), 0, (hipStream_t)stream,
                     cloud, C, offset, count, boxes, nbox, votes_out);
  return (int)hipGetLastError();
}
