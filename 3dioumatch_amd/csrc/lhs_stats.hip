// 3dioumatch_amd/csrc/lhs_stats.hip -- the `view_stats` logging of the semi-supervised step, gfx950.
//
// What it replaces: the view_stats branches of get_pseudo_labels
// (models/loss_helper_unlabeled.py:392-414, :525-553) and of get_pseudo_detection_loss with
// compute_objectness_gt (:82-134, :318-320, :354-359): two all-pairs compute_iou_labels calls
// (models/loss_helper_iou.py:52-112, forward and reverse=True) and about 60 tensor operations over
// their results, several of them boolean-mask writes.  Ground truth is read, never written; the
// pass feeds no loss.
//
//   stats_tile_kernel    grid (ceil(K/16) + 4, S), 256 lanes:
//                        proposal tiles -- 16 teacher proposals x the 64 GT boxes of their scene, a
//                        lane per (proposal, GT column), as scene_max_kernel (iou3d.hip): best IoU and
//                        its first GT index, then per proposal its objectness against the
//                        un-augmented GT centres, its predicted IoU and class, and the student's
//                        objectness against the GT centres in the student's frame;
//                        coverage tiles -- 16 GT boxes x the 64 pseudo-label slots (slot -> proposal
//                        by the filter's own rank, pseudo_rank.h), IoU(GT, slot) of the slots the NMS
//                        kept, its maximum, > 0.25 / > 0.5.
//   stats_reduce_kernel  ONE workgroup: every sum in a fixed order (lane-strided, scene by scene, then
//                        one tree), the twelve scalars.  No float atomics: the result is the same on
//                        every run.
//
// The IoU is iou3d_pair.h's (the code of boxes_iou3d_gpu / the per-scene IoU labels of the loss), the
// box decoding the tensor version's in fp32 (losses.compute_iou_labels): a proposal's IoU label and
// its GT index are bit-identical to what the tensor mirror computes with those kernels.
#include "common.h"
#include "box_geom.h"
#include "iou3d_pair.h"
#include "pseudo_rank.h"
#include "../../include/lhs_hip.h"

namespace {

constexpr int kSlots = 64;       // MAX_NUM_OBJ: pseudo-label slots per scene
constexpr int kGt = 64;          // GT slots per scene
constexpr int kMaxK = 1024;
constexpr int kTile = 16;        // proposals (or GT boxes) per tile
constexpr int kCovTiles = kGt / kTile;
constexpr float kNear = 0.3f, kFar = 0.6f;   // NEAR_THRESHOLD, FAR_THRESHOLD

using boxgeom::BoxPre;
using iou3d_pair::kPolySlots;
using iou3d_pair::LdsPoly;

// per-proposal results of the tile kernel, read by the reduction
struct Ws {
  int *assign;     // (S,K) first GT index of the best IoU
  int *cls;        // (S,K) arg-max class of the teacher
  int *flags;      // (S,K) bit 0: teacher objectness label; bit 1: student objectness mask;
                   //       bit 2: student arg-max == its label, inside the mask
  float *absdiff;  // (S,K) |predicted IoU - IoU label|
  int *slot;       // (S,64) proposal in each pseudo-label slot
  int *cov;        // (S,4,2) GT boxes covered at 0.25 / 0.5, per coverage tile
};

__host__ __device__ inline size_t ws_bytes(int S, int K) {
  const size_t n = (size_t)S * K;
  return sizeof(int) * (4 * n + (size_t)S * kSlots + (size_t)S * kCovTiles * 2);
}

__host__ __device__ inline Ws ws_of(void *p, int S, int K) {
  const size_t n = (size_t)S * K;
  Ws w;
  w.assign = (int *)p;
  w.cls = w.assign + n;
  w.flags = w.cls + n;
  w.absdiff = (float *)(w.flags + n);
  w.slot = (int *)(w.absdiff + n);
  w.cov = w.slot + (size_t)S * kSlots;
  return w;
}

__device__ __forceinline__ int clamp_index(long long v, int n) {
  return v < 0 ? 0 : (v >= n ? n - 1 : (int)v);
}

__device__ __forceinline__ float class2angle(int cls, float residual, int nh) {  // config.class2angle_gpu
  if (nh == 1) return 0.0f;
  const float per = (float)(2.0 * M_PI / (double)nh);
  float angle = (float)cls * per + residual;
  if (angle > (float)M_PI) angle = angle - (float)(2.0 * M_PI);
  return angle;
}

// teacher proposal k of scene s as compute_iou_labels decodes it (loss_helper_iou.py:60-96):
// arg-max heading / size class, their residuals, sizes <= 0 -> 1e-6, heading negated
__device__ __forceinline__ void decode_teacher(const LhsStatsArgs &a, int s, int k, float *o) {
  const long long sk = (long long)s * a.K + k;
  const int hc = pseudo_rank::first_max(a.heading_scores + sk * a.NH, a.NH);
  const int sc = pseudo_rank::first_max(a.size_scores + sk * a.NS, a.NS);
  const float h_res = a.heading_residuals[sk * a.NH + hc];
  for (int d = 0; d < 3; ++d) {
    o[d] = a.center[sk * 3 + d];
    float sz = a.mean_size[sc * 3 + d] + a.size_residuals[(sk * a.NS + sc) * 3 + d];
    if (sz <= 0.0f) sz = 1e-6f;
    o[3 + d] = sz;
  }
  o[6] = -class2angle(hc, h_res, a.NH);
}

// GT box g of label row `row` (losses._gt_boxes): empty slots moved to -1000
__device__ __forceinline__ void decode_gt(const LhsStatsArgs &a, int row, int g, float *o) {
  const long long i = (long long)row * kGt + g;
  const bool empty = a.gt_box_mask[i] != 1.0f;
  const int sc = clamp_index(a.gt_size_class[i], a.NS);
  for (int d = 0; d < 3; ++d) {
    o[d] = empty ? -1000.0f : a.gt_center[i * 3 + d];
    o[3 + d] = a.mean_size[sc * 3 + d] + a.gt_size_residual[i * 3 + d];
  }
  o[6] = -class2angle(clamp_index(a.gt_heading_class[i], a.NH), a.gt_heading_residual[i], a.NH);
}

__device__ __forceinline__ void prepare(const float *bx, float *raw, BoxPre &pre) {
  for (int d = 0; d < 7; ++d) raw[d] = bx[d];
  boxgeom::box_prepare(bx, pre);
}

// squared distance from p to the nearest of the 64 centres, over the 16 lanes of a row: lane c takes
// centres c, c + 16, ...; a minimum is exact in any order
__device__ __forceinline__ float nearest_sq(const float *p, const float *centres, int cidx) {
  float best = INFINITY;
  for (int g = cidx; g < kGt; g += kTile) {
    const float d = sqdist3(p[0], p[1], p[2], centres[g * 3], centres[g * 3 + 1], centres[g * 3 + 2]);
    best = d < best ? d : best;
  }
#pragma unroll
  for (int off = 8; off >= 1; off >>= 1) {
    const float o = __shfl_xor(best, off, 16);
    best = o < best ? o : best;
  }
  return best;
}

__global__ void __launch_bounds__(256) stats_tile_kernel(LhsStatsArgs a, Ws w) {
  __shared__ float poly[kPolySlots * 256];
  __shared__ BoxPre pre[2 * kTile];
  __shared__ float raw[2 * kTile * 7];
  __shared__ float keys[kMaxK];
  __shared__ int slot_of[kSlots];
  __shared__ float gt_teacher[kGt * 3], gt_student[kGt * 3];
  __shared__ int covered[2];
  const int tid = threadIdx.x, s = blockIdx.y;
  const int row_gt = a.labeled + s;
  const int tiles = (a.K + kTile - 1) / kTile;
  const int r = tid >> 4, cidx = tid & 15;
  LdsPoly st{poly + tid};
  float bx[7];

  if ((int)blockIdx.x < tiles) {
    // ---- proposal tile: 16 teacher proposals x 64 GT boxes ----
    const int row0 = blockIdx.x * kTile, gi = row0 + r;
    if (tid < kGt) {
      // GT centres: teacher frame with -1000 placeholders (compute_iou_labels :56-58); student
      // frame = trans_center of the raw label (flips, bmm with rot_mat^T, scale), THEN -1000
      // placeholders (get_unlabeled_loss :573-578, compute_objectness_gt :100-104)
      const long long i = (long long)row_gt * kGt + tid;
      const bool empty = a.gt_box_mask[i] != 1.0f;
      float x = a.gt_center[i * 3], y = a.gt_center[i * 3 + 1];
      const float z = a.gt_center[i * 3 + 2];
      gt_teacher[tid * 3] = empty ? -1000.0f : x;
      gt_teacher[tid * 3 + 1] = empty ? -1000.0f : y;
      gt_teacher[tid * 3 + 2] = empty ? -1000.0f : z;
      x = a.flip_x[s] != 0 ? -x : x;
      y = a.flip_y[s] != 0 ? -y : y;
      const float *R = a.rot_mat + (long long)s * 9;
      const float *sc = a.scale + (long long)s * 3;
      for (int j = 0; j < 3; ++j)
        gt_student[tid * 3 + j] =
            empty ? -1000.0f : ((x * R[j * 3] + y * R[j * 3 + 1]) + z * R[j * 3 + 2]) * sc[j];
    }
    float best = -1.f;  // every IoU is >= 0, so column 0 wins an all-zero row
    int arg = 0;
    for (int col0 = 0; col0 < kGt; col0 += kTile) {
      __syncthreads();
      if (tid < kTile && col0 == 0) {
        decode_teacher(a, s, row0 + tid < a.K ? row0 + tid : a.K - 1, bx);
        prepare(bx, raw + tid * 7, pre[tid]);
      } else if (tid >= kTile && tid < 2 * kTile) {
        decode_gt(a, row_gt, col0 + tid - kTile, bx);
        prepare(bx, raw + tid * 7, pre[tid]);
      }
      __syncthreads();
      if (gi < a.K) {
        const float v = iou3d_pair::iou3d(raw + r * 7, raw + (kTile + cidx) * 7, pre[r],
                                          pre[kTile + cidx], st);
        if (v > best) { best = v; arg = col0 + cidx; }  // strict: the earlier column keeps a tie
      }
    }
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) {  // the 16 lanes of a row: (value desc, index asc)
      const float ov = __shfl_xor(best, off, 16);
      const int oa = __shfl_xor(arg, off, 16);
      if (ov > best || (ov == best && oa < arg)) { best = ov; arg = oa; }
    }
    // nearest GT centres of the teacher's and the student's aggregated vote (all 16 lanes of the row)
    const long long sk = (long long)s * a.K + (gi < a.K ? gi : a.K - 1);
    const float t_sq = nearest_sq(a.vote_xyz + sk * 3, gt_teacher, cidx);
    const float s_sq = nearest_sq(a.student_vote_xyz + sk * 3, gt_student, cidx);
    if (cidx != 0 || gi >= a.K) return;
    const float iou = best < 0.f ? 0.f : best;
    int cls;
    float pred;
    (void)pseudo_rank::key(a.objectness, a.sem_cls, a.iou, a.NC, a.NI, sk, a.obj_threshold,
                           a.cls_threshold, a.iou_threshold, &cls, &pred);
    // teacher objectness: aggregated vote within 0.3 of a GT centre (compute_iou_labels :69-74)
    const int t_obj = sqrtf(t_sq + 1e-6f) < kNear ? 1 : 0;
    // student: compute_objectness_gt's label / mask and the arg-max of its objectness (:354-359)
    const float dist = sqrtf(s_sq + 1e-6f);
    const int s_label = dist < kNear ? 1 : 0;
    const int s_mask = (dist < kNear || dist > kFar) ? 1 : 0;
    const int s_pred = a.student_objectness[sk * 2 + 1] > a.student_objectness[sk * 2] ? 1 : 0;
    a.iou_labels[sk] = iou;
    w.assign[sk] = arg;
    w.cls[sk] = cls;
    w.flags[sk] = t_obj | (s_mask << 1) | ((s_mask && s_pred == s_label) ? 4 : 0);
    w.absdiff[sk] = fabsf(pred - iou);
    return;
  }

  // ---- coverage tile: 16 GT boxes x the 64 pseudo-label slots (reverse=True: GT box first) ----
  const int q = blockIdx.x - tiles;
  for (int k = tid; k < a.K; k += 256) {
    int cls;
    float pred;
    keys[k] = pseudo_rank::key(a.objectness, a.sem_cls, a.iou, a.NC, a.NI, (long long)s * a.K + k,
                               a.obj_threshold, a.cls_threshold, a.iou_threshold, &cls, &pred);
  }
  if (tid < kSlots) slot_of[tid] = 0;
  if (tid < 2) covered[tid] = 0;
  __syncthreads();
  for (int k = tid; k < a.K; k += 256) {
    const int rk = pseudo_rank::rank(keys, a.K, k);
    if (rk < kSlots) slot_of[rk] = k;
  }
  __syncthreads();
  if (q == 0 && tid < kSlots) w.slot[(long long)s * kSlots + tid] = slot_of[tid];
  const int g = q * kTile + r;
  float best = 0.f;  // max over slots of IoU * label_mask: 0 for a slot the NMS dropped
  for (int col0 = 0; col0 < kSlots; col0 += kTile) {
    __syncthreads();
    if (tid < kTile && col0 == 0) {
      decode_gt(a, row_gt, q * kTile + tid, bx);
      prepare(bx, raw + tid * 7, pre[tid]);
    } else if (tid >= kTile && tid < 2 * kTile) {
      decode_teacher(a, s, slot_of[col0 + tid - kTile], bx);
      prepare(bx, raw + tid * 7, pre[tid]);
    }
    __syncthreads();
    const int j = col0 + cidx;
    if (a.label_mask[(long long)s * kSlots + j] != 0) {
      const float v = iou3d_pair::iou3d(raw + r * 7, raw + (kTile + cidx) * 7, pre[r],
                                        pre[kTile + cidx], st);
      best = v > best ? v : best;
    }
  }
#pragma unroll
  for (int off = 8; off >= 1; off >>= 1) {
    const float ov = __shfl_xor(best, off, 16);
    best = ov > best ? ov : best;
  }
  const bool lead = cidx == 0 && g < kGt;
  const unsigned long long b25 = __ballot(lead && best > 0.25f);
  const unsigned long long b50 = __ballot(lead && best > 0.5f);
  if (lane_id() == 0) {  // integer LDS atomics: the count does not depend on their order
    atomicAdd(&covered[0], (int)__popcll(b25));
    atomicAdd(&covered[1], (int)__popcll(b50));
  }
  __syncthreads();
  if (tid < 2) w.cov[((long long)s * kCovTiles + q) * 2 + tid] = covered[tid];
}

constexpr int kReduceLanes = 256;
constexpr int kFloatSums = 7, kIntSums = 9;

__global__ void __launch_bounds__(kReduceLanes) stats_reduce_kernel(LhsStatsArgs a, Ws w) {
  __shared__ float fs[kFloatSums][kReduceLanes];
  __shared__ int is[kIntSums][kReduceLanes];
  const int tid = threadIdx.x;
  // f: IoU, IoU * obj, |err|, |err| * obj, slot IoU * mask, slot IoU * mask * obj, GT boxes of all rows
  // n: obj, student mask, student correct, mask, mask * obj, class right * mask, ... * obj, covered x2
  float f[kFloatSums] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int n[kIntSums] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int s = 0; s < a.S; ++s) {   // scene by scene, each lane in the same order on every run
    for (int k = tid; k < a.K; k += kReduceLanes) {
      const long long sk = (long long)s * a.K + k;
      const float iou = a.iou_labels[sk], err = w.absdiff[sk];
      const int fl = w.flags[sk], obj = fl & 1;
      f[0] += iou;
      f[1] += obj ? iou : 0.0f;
      f[2] += err;
      f[3] += obj ? err : 0.0f;
      n[0] += obj;
      n[1] += (fl >> 1) & 1;
      n[2] += (fl >> 2) & 1;
    }
    if (tid < kSlots) {  // the 64 slots after the NMS (get_pseudo_labels :525-546)
      const long long slot = (long long)s * kSlots + tid;
      const int m = a.label_mask[slot] != 0 ? 1 : 0;
      const long long sk = (long long)s * a.K + clamp_index(w.slot[slot], a.K);
      const float iou = a.iou_labels[sk];
      const int obj = w.flags[sk] & 1;
      const long long gt = (long long)(a.labeled + s) * kGt + clamp_index(w.assign[sk], kGt);
      const int right = (long long)w.cls[sk] == a.gt_sem_cls[gt] ? 1 : 0;
      f[4] += m ? iou : 0.0f;
      f[5] += (m && obj) ? iou : 0.0f;
      n[3] += m;
      n[4] += m & obj;
      n[5] += m & right;
      n[6] += m & right & obj;
    }
    if (tid < kCovTiles) {
      n[7] += w.cov[((long long)s * kCovTiles + tid) * 2];
      n[8] += w.cov[((long long)s * kCovTiles + tid) * 2 + 1];
    }
  }
  for (long long i = tid; i < (long long)a.rows * kGt; i += kReduceLanes) f[6] += a.gt_box_mask[i];
  for (int v = 0; v < kFloatSums; ++v) fs[v][tid] = f[v];
  for (int v = 0; v < kIntSums; ++v) is[v][tid] = n[v];
  __syncthreads();
  for (int off = kReduceLanes / 2; off > 0; off >>= 1) {
    if (tid < off) {
      for (int v = 0; v < kFloatSums; ++v) fs[v][tid] += fs[v][tid + off];
      for (int v = 0; v < kIntSums; ++v) is[v][tid] += is[v][tid + off];
    }
    __syncthreads();
  }
  if (tid != 0) return;
  const float all = (float)((long long)a.S * a.K);
  const float n_obj = (float)is[0][0] + 1e-6f, n_m = (float)is[3][0] + 1e-6f;
  const float n_mobj = (float)is[4][0] + 1e-6f, gt_count = fs[6][0];
  float *o = a.stats;
  o[LHS_STAT_PRED_IOU] = fs[0][0] / all;
  o[LHS_STAT_PRED_IOU_OBJ] = fs[1][0] / n_obj;
  o[LHS_STAT_IOU_ACC] = fs[2][0] / all;
  o[LHS_STAT_IOU_OBJ_ACC] = fs[3][0] / n_obj;
  o[LHS_STAT_FINAL_IOU] = fs[4][0] / n_m;
  o[LHS_STAT_FINAL_IOU_OBJ] = fs[5][0] / n_mobj;
  o[LHS_STAT_FINAL_CLS] = (float)is[5][0] / n_m;
  o[LHS_STAT_FINAL_CLS_OBJ] = (float)is[6][0] / n_mobj;
  o[LHS_STAT_COVERAGE_25] = (float)is[7][0] / gt_count;   // over the GT boxes of ALL rows, as the
  o[LHS_STAT_COVERAGE_50] = (float)is[8][0] / gt_count;   // reference divides (:530, :551-552)
  const float acc = (float)is[2][0] / ((float)is[1][0] + 1e-6f);
  o[LHS_STAT_TRUE_OBJ_ACC] = acc;
  o[LHS_STAT_OBJ_ACC] = acc;
}

bool valid(const LhsStatsArgs *a) {
  if (!a || a->S <= 0 || a->S > 65535 || a->K < kSlots || a->K > kMaxK || a->NC <= 0 ||
      (a->NI != 1 && a->NI != a->NC) || a->NH <= 0 || a->NS <= 0 || a->labeled < 0 ||
      a->rows != a->labeled + a->S)
    return false;
  const void *ptrs[] = {a->objectness, a->sem_cls, a->iou, a->heading_scores, a->heading_residuals,
                        a->size_scores, a->size_residuals, a->center, a->vote_xyz, a->mean_size,
                        a->label_mask, a->gt_center, a->gt_heading_class, a->gt_heading_residual,
                        a->gt_size_class, a->gt_size_residual, a->gt_sem_cls, a->gt_box_mask,
                        a->student_objectness, a->student_vote_xyz, a->flip_x, a->flip_y, a->rot_mat,
                        a->scale, a->iou_labels, a->stats, a->workspace};
  for (const void *p : ptrs)
    if (!p) return false;
  return true;
}

}  // namespace

extern "C" __attribute__((visibility("default")))
size_t lhs_pseudo_stats_workspace_bytes(int S, int K) {
  return S > 0 && K > 0 ? ws_bytes(S, K) : 0;
}

extern "C" __attribute__((visibility("default")))
int lhs_pseudo_stats(const LhsStatsArgs *args, void *stream) {
  if (!valid(args)) return (int)hipErrorInvalidValue;
  const Ws w = ws_of(args->workspace, args->S, args->K);
  const int tiles = (args->K + kTile - 1) / kTile;
  hipLaunchKernelGGL(stats_tile_kernel, dim3(tiles + kCovTiles, args->S), dim3(256), 0,
                     (hipStream_t)stream, *args, w);
  int rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  hipLaunchKernelGGL(stats_reduce_kernel, dim3(1), dim3(kReduceLanes), 0, (hipStream_t)stream, *args, w);
  return (int)hipGetLastError();
}
