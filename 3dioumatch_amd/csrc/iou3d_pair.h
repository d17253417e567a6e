// 3dioumatch_amd/csrc/iou3d_pair.h -- the 3-D IoU of one box pair on gfx950, shared by the kernels
// that need it (iou3d.hip: all-pairs matrix, per-scene best match; lhs_stats.hip: the view_stats
// IoU labels), so that every IoU the step logs or trains on is the same sequence of fp32 operations.
//
// Semantics: boxes_iou3d_gpu's epilogue (iou3d_nms_utils.py:60-79) around the reference's BEV
// overlap (iou3d_nms_kernel.cu:105-226, box_geom.h).
#pragma once
#include "box_geom.h"

namespace iou3d_pair {

constexpr int kPolySlots = boxgeom::kMaxPoly * 3;  // x, y, angle per vertex

// polygon store in LDS: element (slot s, lane t) at base[s*256 + t]
struct LdsPoly {
  float *base;
  __device__ __forceinline__ float &x(int i) { return base[(i * 3 + 0) * 256]; }
  __device__ __forceinline__ float &y(int i) { return base[(i * 3 + 1) * 256]; }
  __device__ __forceinline__ float &a(int i) { return base[(i * 3 + 2) * 256]; }
};

// 3-D IoU of raw boxes a, b (x, y, z, dx, dy, dz, heading) with their BoxPre A, B
__device__ __forceinline__ float iou3d(const float *a, const float *b, const boxgeom::BoxPre &A,
                                       const boxgeom::BoxPre &B, LdsPoly &st) {
  const float a_max = a[2] + a[5] / 2, a_min = a[2] - a[5] / 2;
  const float b_max = b[2] + b[5] / 2, b_min = b[2] - b[5] / 2;
  const float max_of_min = a_min > b_min ? a_min : b_min;
  const float min_of_max = a_max < b_max ? a_max : b_max;
  float h = min_of_max - max_of_min;
  if (h < 0.f) h = 0.f;
  const float ov_bev = h > 0.f ? boxgeom::overlap_area(A, B, st) : 0.f;
  const float ov3d = ov_bev * h;
  const float vol_a = a[3] * a[4] * a[5], vol_b = b[3] * b[4] * b[5];
  float den = vol_a + vol_b - ov3d;
  if (den < 1e-6f) den = 1e-6f;
  return ov3d / den;
}

}  // namespace iou3d_pair
