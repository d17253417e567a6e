// 3dioumatch_amd/csrc/eval_obb_iou.hip -- oriented-box IoU of the AP evaluation on the device
// (gfx950), SURVEY section 8(f) rank 4.
//
// What it replaces: the innermost loops of eval_det_cls (utils/eval_det.py:128-141).  For every
// detection, in score order, the reference calls get_iou_obb = box3d_iou
// (utils/box_util.py:112-137) against each ground-truth box of the same scan and class -- pure
// Python: Sutherland-Hodgman clipping of the two footprints (polygon_clip, box_util.py:23-69), a
// scipy ConvexHull for the area of the clipped polygon (:77-88), the overlap of the vertical
// extents and box3d_vol (:91-96) -- and keeps (ovmax, jmax) under a strict `>` update.  The
// detections are independent of each other until the greedy TP/FP marking, so the IoUs and the
// per-detection maximum are computed here in one launch and only the marking stays on the host.
//
// Arithmetic: float32 corners promoted to float64 (the reference's `.astype(float)`,
// eval_det.py:130-132), every expression evaluated in the reference's order (-ffp-contract=off),
// so the strict inside() tests of the clipping take the same branches.  The area of the clipped
// polygon is the shoelace sum (the polygon is convex, so this is the hull area the reference gets
// from qhull, to rounding); a clipped polygon with fewer than 3 vertices has area 0 (the
// reference raises QhullError there).
//
// One thread per detection (best_match) or per pair (matrix); the polygons live in registers /
// scratch (<= 8 vertices: a quad gains at most one vertex per clipping edge).
#include "eval_box_iou.h"  // box3d_iou / clipped_area / load_box, shared with eval_ap.hip

namespace {

__global__ __launch_bounds__(128)
void corners_iou_matrix_kernel(int n, int m, const float *__restrict__ a,
                               const float *__restrict__ b, double *__restrict__ iou) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (long long)n * m) return;
  float ca[24], cb[24];
  load_box(a + (p / m) * 24, ca);
  load_box(b + (p % m) * 24, cb);
  iou[p] = box3d_iou(ca, cb);
}

// eval_det.py:128-141: ovmax = -inf; for j: if iou > ovmax: ovmax = iou, jmax = j
__global__ __launch_bounds__(128)
void corners_best_match_kernel(int nd, const float *__restrict__ det, const int *__restrict__ gt_begin,
                               const int *__restrict__ gt_count, const float *__restrict__ gt,
                               double *__restrict__ ovmax, int *__restrict__ jmax) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= nd) return;
  float cd[24], cg[24];
  load_box(det + (long long)d * 24, cd);
  const int g0 = gt_begin[d], cnt = gt_count[d];
  double best = -INFINITY;
  int bj = -1;
  for (int j = 0; j < cnt; ++j) {
    load_box(gt + (long long)(g0 + j) * 24, cg);
    const double v = box3d_iou(cd, cg);
    if (v > best) { best = v; bj = j; }
  }
  ovmax[d] = best;
  jmax[d] = bj;
}

}  // namespace

// iou (n,m) f64 <- box3d_iou(a[i], b[j])[0]; a (n,8,3), b (m,8,3) float32 corners
extern "C" __attribute__((visibility("default")))
int iou3d_corners_iou3d(int n, const float *a, int m, const float *b, double *iou, void *stream) {
  if (n < 0 || m < 0) return (int)hipErrorInvalidValue;
  const long long pairs = (long long)n * m;
  if (pairs == 0) return 0;
  if (pairs > 0x7fffffffLL * 128) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(corners_iou_matrix_kernel, dim3((unsigned)((pairs + 127) / 128)), dim3(128), 0,
                     (hipStream_t)stream, n, m, a, b, iou);
  return (int)hipGetLastError();
}

// ovmax (nd) f64, jmax (nd) i32 <- best ground-truth box of det d among gt[gt_begin[d] ..
// gt_begin[d]+gt_count[d]); (-inf, -1) when gt_count[d] == 0
extern "C" __attribute__((visibility("default")))
int iou3d_corners_best_match(int nd, const float *det, const int *gt_begin, const int *gt_count,
                             const float *gt, double *ovmax, int *jmax, void *stream) {
  if (nd < 0) return (int)hipErrorInvalidValue;
  if (nd == 0) return 0;
  hipLaunchKernelGGL(corners_best_match_kernel, dim3((nd + 127) / 128), dim3(128), 0,
                     (hipStream_t)stream, nd, det, gt_begin, gt_count, gt, ovmax, jmax);
  return (int)hipGetLastError();
}
