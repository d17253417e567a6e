// 3dioumatch_amd/csrc/iou_opt.hip -- test-time IoU optimisation of the predicted boxes
// (train.py:444-491 of the reference, evaluate_with_opt): the gradient of the summed IoU logits
// with respect to every box's centre and half size, and the ascent step, as ONE kernel per pass.
//
// The reference (models/grid_conv_module.py:64-105) differentiates through a materialised
// (B, K*64*3, C) gather of seed features and the inverse-distance weights.  Here the layer-0
// gradient dy0 (B, M, K*64) of the IoU branch's shared MLP is contracted against the projected
// seed features P = W0[:, 3:] . F (B, M, Nseed) instead: dL/dw_j = <dy0_g, P[:, idx_gj]>, so the
// C-channel gradient of the interpolated features is never formed.  What remains per grid point
// is the chain rule through the three normalised inverse distances and the box -> grid-point map:
//
//   rel_g = R (u_g * s),  q_g = rel_g + c,  p_j = seed_xyz[idx_gj],  d_j = |q_g - p_j|
//   r_j = 1 / (d_j + 1e-8),  w_j = r_j / sum r,  a_j = <dy0_g, P[:, idx_gj]>
//   dL/dd_j = -r_j^2 (a_j - sum_i a_i w_i) / sum r
//   dq_g = sum_j dL/dd_j (q_g - p_j) / d_j,   drel_g = W0[:, :3]^T dy0_g
//   dc = sum_g dq_g,   ds = sum_g u_g * R^T (dq_g + drel_g)
//
// R = rot_gpu(h) (utils/box_util.py:292-306): R v = (c vx + s vy, c vy - s vx, vz).
// One wave per box, one lane per grid point; the 64-lane sums are butterfly reductions in a fixed
// order (no atomics: the result is bit-identical run to run).
#include "common.h"

namespace {

__global__ void __launch_bounds__(256)
iou_opt_box_step_kernel(int boxes, int k, int nseed, int ch, const float *__restrict__ unit,
                        const float *__restrict__ seed_xyz, const int *__restrict__ idx,
                        const float *__restrict__ proj, const float *__restrict__ w0, int ldw0,
                        const float *__restrict__ dz, const float *__restrict__ y0,
                        const float *__restrict__ scale, const float *__restrict__ shift,
                        const float *__restrict__ gain, const float *__restrict__ heading, float rate,
                        float *__restrict__ center, float *__restrict__ size, float *__restrict__ grad) {
  const int box = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (box >= boxes) return;  // uniform per wave
  const int g = threadIdx.x & 63, b = box / k, kk = box - b * k;
  const size_t cols = (size_t)k * 64, col = (size_t)kk * 64 + g;

  const float ux = unit[g * 3 + 0], uy = unit[g * 3 + 1], uz = unit[g * 3 + 2];
  const float sx = size[box * 3 + 0], sy = size[box * 3 + 1], sz = size[box * 3 + 2];
  const float cx = center[box * 3 + 0], cy = center[box * 3 + 1], cz = center[box * 3 + 2];
  const float h = heading[box];
  const float cs = cosf(h), sn = sinf(h);
  const float lx = ux * sx, ly = uy * sy, lz = uz * sz;
  const float qx = lx * cs + ly * sn + cx, qy = ly * cs - lx * sn + cy, qz = lz + cz;

  const int *ig = idx + ((size_t)b * cols + col) * 3;
  int nb[3];
  float dx[3], dy[3], dzz[3], d[3], r[3];
  float rsum = 0.f;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    nb[j] = ig[j];
    const float *p = seed_xyz + ((size_t)b * nseed + nb[j]) * 3;
    dx[j] = qx - p[0]; dy[j] = qy - p[1]; dzz[j] = qz - p[2];
    d[j] = sqrtf(dx[j] * dx[j] + dy[j] * dy[j] + dzz[j] * dzz[j]);
    r[j] = 1.f / (d[j] + 1e-8f);
    rsum += r[j];
  }

  // a_j = <dy0_g, P[:, idx_gj]> and drel = W0[:, :3]^T dy0_g in one pass over the M channels;
  // dy0 = dz * gain * [y0 * scale + shift > 0] (eval-mode BatchNorm + ReLU backward) where y0 is given
  const float *dzc = dz + (size_t)b * ch * cols + col;
  const float *yc = y0 ? y0 + (size_t)b * ch * cols + col : nullptr;
  const float *pc = proj + (size_t)b * ch * nseed;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, rx = 0.f, ry = 0.f, rz = 0.f;
#pragma unroll 4
  for (int m = 0; m < ch; ++m) {
    float gy = dzc[(size_t)m * cols];
    if (yc) gy = __fmaf_rn(yc[(size_t)m * cols], scale[m], shift[m]) > 0.f ? gain[m] * gy : 0.f;
    const float *pm = pc + (size_t)m * nseed;
    a0 = __fmaf_rn(gy, pm[nb[0]], a0);
    a1 = __fmaf_rn(gy, pm[nb[1]], a1);
    a2 = __fmaf_rn(gy, pm[nb[2]], a2);
    const float *wm = w0 + (size_t)m * ldw0;
    rx = __fmaf_rn(gy, wm[0], rx);
    ry = __fmaf_rn(gy, wm[1], ry);
    rz = __fmaf_rn(gy, wm[2], rz);
  }
  const float inv = 1.f / rsum;
  const float abar = (a0 * r[0] + a1 * r[1] + a2 * r[2]) * inv;  // sum_i a_i w_i
  const float aj[3] = {a0, a1, a2};
  float gqx = 0.f, gqy = 0.f, gqz = 0.f;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    // a grid point exactly on a seed: the reference's sqrt has no finite derivative there; the
    // point contributes nothing through that neighbour instead of a NaN
    if (d[j] > 0.f) {
      const float gd = -(r[j] * r[j]) * (aj[j] - abar) * inv;
      const float t = gd / d[j];
      gqx += t * dx[j]; gqy += t * dy[j]; gqz += t * dzz[j];
    }
  }
  // R^T (dq + drel), then the unit-grid factor of the half size
  const float vx = gqx + rx, vy = gqy + ry, vz = gqz + rz;
  const float tx = cs * vx - sn * vy, ty = sn * vx + cs * vy;
  const float dcx = wave_sum(gqx), dcy = wave_sum(gqy), dcz = wave_sum(gqz);
  const float dsx = wave_sum(ux * tx), dsy = wave_sum(uy * ty), dsz = wave_sum(uz * vz);
  if (g == 0) {
    if (grad) {
      float *o = grad + (size_t)box * 6;
      o[0] = dcx; o[1] = dcy; o[2] = dcz; o[3] = dsx; o[4] = dsy; o[5] = dsz;
    }
    center[box * 3 + 0] = cx + rate * dcx;
    center[box * 3 + 1] = cy + rate * dcy;
    center[box * 3 + 2] = cz + rate * dcz;
    size[box * 3 + 0] = sx + rate * dsx;
    size[box * 3 + 1] = sy + rate * dsy;
    size[box * 3 + 2] = sz + rate * dsz;
  }
}

}  // namespace

PN2_API int votenet_iou_opt_box_step(int b, int k, int nseed, int ch, const float *unit,
                                     const float *seed_xyz, const int *idx, const float *proj,
                                     const float *w0, int ldw0, const float *dz, const float *y0,
                                     const float *scale, const float *shift, const float *gain,
                                     const float *heading, float rate, float *center, float *size,
                                     float *grad, void *stream_) {
  if (b <= 0 || k <= 0) return 0;
  if (nseed <= 0 || ch <= 0 || ldw0 < 3 || !unit || !seed_xyz || !idx || !proj || !w0 || !dz ||
      !heading || !center || !size)
    return (int)hipErrorInvalidValue;
  if (y0 && (!scale || !shift || !gain)) return (int)hipErrorInvalidValue;
  const long long boxes = (long long)b * k;
  if (boxes * 64 > 0x7fffffffll) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(iou_opt_box_step_kernel, dim3(pn2_ceil_div(boxes, 4)), dim3(256), 0,
                     (hipStream_t)stream_, (int)boxes, k, nseed, ch, unit, seed_xyz, idx, proj, w0,
                     ldw0, dz, y0, scale, shift, gain, heading, rate, center, size, grad);
  return pn2_launch_status();
}
