// 3dioumatch_amd/csrc/box_points.hip -- points inside every predicted box (gfx950).
//
// What it replaces: the `remove_empty_box` filter of parse_predictions (models/ap_helper.py:123-135):
// B x K host calls of extract_pc_in_box3d (sunrgbd/sunrgbd_utils.py:215-224), each one scipy
// Delaunay triangulation of the box's eight corners and one find_simplex over all N points of the
// scene.  The hull of get_3d_box(size, heading, flip_axis_to_camera(center)) flipped back to the
// depth frame is an upright box turned about z, so membership is the closed-form test
//
//   d = p - center,  x' = c d.x - s d.y,  z' = s d.x + c d.y   (c = cos heading, s = sin heading)
//   inside  <=>  |x'| <= l/2  and  |z'| <= w/2  and  |d.z| <= h/2
//
// One lane per box: its frame (c, s, centre, half sizes) is computed once in float64, rounded to
// float32 and kept in eight registers.  A workgroup stages one chunk of kBoxPointChunk points in LDS
// as float4; every lane then reads the same address (a broadcast, no bank conflict) and counts in a
// register.  One integer atomicAdd per (lane, chunk) with a non-zero count lands in `count`, which
// the entry point zero-fills first: integer sums do not depend on arrival order, so the result is
// deterministic.  Per-pair arithmetic is float32, every operation rounded (no a*b+c contraction).
#include "common.h"

namespace {

constexpr int kBoxPointChunk = 512;   // points per workgroup (votenet/pseudo_nms.py BOX_POINT_CHUNK)
constexpr int kBoxPointLanes = 256;   // boxes per workgroup
constexpr int kBoxPointBatch = 8;     // points read from LDS ahead of their tests (divides the chunk)

__global__ void __launch_bounds__(kBoxPointLanes)
box_point_count_kernel(int n, int npts, int pstride, int chunks, const float *__restrict__ points,
                       const float *__restrict__ center, const double *__restrict__ size,
                       const double *__restrict__ heading, int *__restrict__ count) {
  __shared__ float4 s_pt[kBoxPointChunk];
  const int scene = blockIdx.y, tid = threadIdx.x;
  const int chunk = blockIdx.x % chunks, box = (blockIdx.x / chunks) * kBoxPointLanes + tid;
  const int p0 = chunk * kBoxPointChunk;
  const int cnt = npts - p0 < kBoxPointChunk ? npts - p0 : kBoxPointChunk;
  const float *src = points + ((size_t)scene * npts + p0) * pstride;
  // the chunk's tail up to a multiple of kBoxPointBatch is padded with NaN points: inside no box
  const int padded = (cnt + kBoxPointBatch - 1) / kBoxPointBatch * kBoxPointBatch;
  for (int k = tid; k < padded; k += kBoxPointLanes) {
    const float *p = src + (size_t)k * pstride;
    const float nan = __int_as_float(0x7fc00000);
    s_pt[k] = k < cnt ? make_float4(p[0], p[1], p[2], 0.f) : make_float4(nan, nan, nan, 0.f);
  }
  __syncthreads();
  if (box >= n) return;
  const size_t b = (size_t)scene * n + box;
  const double ang = heading[b];
  const float c = (float)cos(ang), s = (float)sin(ang);
  const float cx = center[b * 3 + 0], cy = center[b * 3 + 1], cz = center[b * 3 + 2];
  const float hl = (float)(size[b * 3 + 0] / 2), hw = (float)(size[b * 3 + 1] / 2),
              hh = (float)(size[b * 3 + 2] / 2);
  int inside = 0;
  for (int k0 = 0; k0 < padded; k0 += kBoxPointBatch) {
    float4 p[kBoxPointBatch];   // all the batch's LDS reads in flight before the first use
#pragma unroll
    for (int k = 0; k < kBoxPointBatch; ++k) p[k] = s_pt[k0 + k];
#pragma unroll
    for (int k = 0; k < kBoxPointBatch; ++k) {
      const float dx = __fsub_rn(p[k].x, cx), dy = __fsub_rn(p[k].y, cy), dz = __fsub_rn(p[k].z, cz);
      const float xr = __fsub_rn(__fmul_rn(c, dx), __fmul_rn(s, dy));
      const float zr = __fadd_rn(__fmul_rn(s, dx), __fmul_rn(c, dy));
      // `&`, not `&&`: three compares and two mask ands, no branch per point
      inside += (int)(fabsf(xr) <= hl) & (int)(fabsf(zr) <= hw) & (int)(fabsf(dz) <= hh);
    }
  }
  if (inside) atomicAdd(count + b, inside);
}

}  // namespace

// count (scenes, n) int32 <- number of points of the scene inside each oriented box: what
// len(extract_pc_in_box3d(pc, flip_axis_to_depth(corners))[0]) is in models/ap_helper.py:123-135
// (sunrgbd/sunrgbd_utils.py:215-224).  points (scenes, npts, pstride) f32 with xyz first.
extern "C" __attribute__((visibility("default")))
int lhs_box_point_count(int scenes, int n, int npts, int pstride, const float *points,
                        const float *center, const double *size, const double *heading, int *count,
                        void *stream) {
  if (scenes <= 0 || n <= 0 || npts <= 0) return 0;
  const long long chunks = pn2_ceil_div(npts, kBoxPointChunk);
  const long long blocks = chunks * pn2_ceil_div(n, kBoxPointLanes);
  if (pstride < 3 || blocks > 0x7fffffffLL || scenes > 65535) return (int)hipErrorInvalidValue;
  const int st = pn2_zero_async(count, (size_t)scenes * n * sizeof(int), (hipStream_t)stream);
  if (st != 0) return st;
  hipLaunchKernelGGL(box_point_count_kernel, dim3((unsigned)blocks, (unsigned)scenes),
                     dim3(kBoxPointLanes), 0, (hipStream_t)stream, n, npts, pstride, (int)chunks,
                     points, center, size, heading, count);
  return pn2_launch_status();
}
