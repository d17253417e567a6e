// 3dioumatch_amd/csrc/feat_norm.hip -- unit-length vote features.
//
// What it replaces: models/votenet_iou_branch.py:103-104,
//     features_norm = torch.norm(features, p=2, dim=1); features = features.div(features_norm.unsqueeze(1))
// and its autograd backward (about thirty element-wise / reduction kernels over a (B, 256, 1024)
// tensor in the training step).  One kernel each way:
//     forward : norm[b][j] = sqrt(sum_c x[b][c][j]^2),  y = x / norm
//     backward: dx = (dy - y * sum_c(dy * y)) / norm
// A workgroup owns 64 columns of one cloud; its 4 waves split the channels, partial sums meet in
// LDS.  No epsilon, as in the reference (a zero column gives the same NaNs).
#include "common.h"

namespace {

// sum over channels of f(channel value(s)) for column j, channels split over the 4 waves
template <bool GRAD>
__global__ void __launch_bounds__(256)
channel_normalize_kernel(int c, int n, const float *__restrict__ x, const float *__restrict__ dy,
                         float *__restrict__ norm, float *__restrict__ out) {
  __shared__ float part[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + lane, b = blockIdx.y;
  const bool live = j < n;
  const size_t base = (size_t)b * c * n + (live ? j : 0);
  const int c_lo = (int)((long long)c * wave / 4), c_hi = (int)((long long)c * (wave + 1) / 4);
  float acc = 0.f;
  if (live) {
    // eight rows in flight per lane (128 workgroups x 4 waves with one 256-byte load each in
    // flight left the kernel at 0.6 TB/s); the sum keeps its channel order
    int ch = c_lo;
    for (; ch + 8 <= c_hi; ch += 8) {
      float v[8], g[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        v[u] = x[base + (size_t)(ch + u) * n];  // forward: x; backward: y
        g[u] = GRAD ? dy[base + (size_t)(ch + u) * n] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += GRAD ? g[u] * v[u] : v[u] * v[u];
    }
    for (; ch < c_hi; ++ch) {
      const float v = x[base + (size_t)ch * n];
      acc += GRAD ? dy[base + (size_t)ch * n] * v : v * v;
    }
  }
  part[wave][lane] = acc;
  __syncthreads();
  const float total = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
  if (!live) return;
  if (!GRAD) {
    const float len = sqrtf(total);
    if (wave == 0) norm[(size_t)b * n + j] = len;
#pragma unroll 8
    for (int ch = c_lo; ch < c_hi; ++ch) out[base + (size_t)ch * n] = x[base + (size_t)ch * n] / len;
  } else {
    const float len = norm[(size_t)b * n + j];
#pragma unroll 8
    for (int ch = c_lo; ch < c_hi; ++ch) {
      const size_t o = base + (size_t)ch * n;
      out[o] = (dy[o] - x[o] * total) / len;
    }
  }
}

// channel_normalize_kernel with the voting module's tail (models/voting_module.py:52-63) on both
// sides of it, one launch each way.  Same channel split over the four waves, same 8-row groups,
// same (p0 + p1) + (p2 + p3) combination: every element is computed as the separate kernels did.
//   forward : f = seed_features + net[:, 3:] (added on load), norm = ||f||_2, vote_features = f / norm,
//             vote_xyz[b][j][d] = seed_xyz[b][j][d] + net[b][d][j]
//   backward: dx = (dy - y * sum_c(dy * y)) / norm  -> d_net[:, 3:] and d_seed_features,
//             g_xyz (b,n,3) transposed -> d_net[:, :3], and as it is -> d_seed_xyz
// x: seed_features / y (b,c,n); r: net (b,3+c,n) / dy (b,c,n); xyz: seed_xyz / g_xyz (b,n,3; g_xyz
// may be null = zeros); out: vote_features (b,c,n) / d_net (b,3+c,n); out_xyz: vote_xyz / d_seed_xyz
// (b,n,3; the latter may be null); out2: d_seed_features (b,c,n; backward only, may be null).
template <bool GRAD>
__global__ void __launch_bounds__(256)
vote_tail_kernel(int c, int n, const float *__restrict__ x, const float *__restrict__ r,
                 const float *__restrict__ xyz, float *__restrict__ norm, float *__restrict__ out,
                 float *__restrict__ out_xyz, float *__restrict__ out2) {
  __shared__ float part[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + lane, b = blockIdx.y;
  const bool live = j < n;
  const size_t base = (size_t)b * c * n + (live ? j : 0);              // (b, c, n) tensors
  const size_t wide = (size_t)b * (3 + c) * n + (live ? j : 0);        // row 0 of the (b, 3+c, n) one
  const size_t rbase = GRAD ? base : wide + 3 * (size_t)n;             // r's row of channel 0
  const int c_lo = (int)((long long)c * wave / 4), c_hi = (int)((long long)c * (wave + 1) / 4);
  float acc = 0.f;
  if (live) {
    int ch = c_lo;
    for (; ch + 8 <= c_hi; ch += 8) {
      float v[8], g[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        v[u] = x[base + (size_t)(ch + u) * n];
        g[u] = r[rbase + (size_t)(ch + u) * n];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (GRAD) {
          acc += g[u] * v[u];
        } else {
          const float f = v[u] + g[u];
          acc += f * f;
        }
      }
    }
    for (; ch < c_hi; ++ch) {
      const float v = x[base + (size_t)ch * n], g = r[rbase + (size_t)ch * n];
      if (GRAD) {
        acc += g * v;
      } else {
        const float f = v + g;
        acc += f * f;
      }
    }
  }
  part[wave][lane] = acc;
  __syncthreads();
  const float total = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
  if (!live) return;
  const size_t p3 = ((size_t)b * n + j) * 3;
  if (!GRAD) {
    const float len = sqrtf(total);
    if (wave == 0) {
      norm[(size_t)b * n + j] = len;
#pragma unroll
      for (int d = 0; d < 3; ++d) out_xyz[p3 + d] = xyz[p3 + d] + r[wide + (size_t)d * n];
    }
#pragma unroll 8
    for (int ch = c_lo; ch < c_hi; ++ch)
      out[base + (size_t)ch * n] = (x[base + (size_t)ch * n] + r[rbase + (size_t)ch * n]) / len;
  } else {
    const float len = norm[(size_t)b * n + j];
    if (wave == 0) {
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const float g = xyz ? xyz[p3 + d] : 0.f;
        out[wide + (size_t)d * n] = g;
        if (out_xyz) out_xyz[p3 + d] = g;
      }
    }
#pragma unroll 8
    for (int ch = c_lo; ch < c_hi; ++ch) {
      const size_t o = base + (size_t)ch * n;
      const float dx = (r[o] - x[o] * total) / len;
      out[wide + (size_t)(3 + ch) * n] = dx;
      if (out2) out2[o] = dx;
    }
  }
}

}  // namespace

// net (b,3+c,n), seed_xyz (b,n,3), seed_features (b,c,n) -> vote_xyz (b,n,3), vote_features (b,c,n)
// of unit length over c, norm (b,n)
PN2_API int votenet_vote_tail(int b, int c, int n, const float *net, const float *seed_xyz,
                              const float *seed_features, float *vote_xyz, float *vote_features,
                              float *norm, void *stream_) {
  if (b <= 0 || c <= 0 || n <= 0) return 0;
  if (!net || !seed_xyz || !seed_features || !vote_xyz || !vote_features || !norm)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(vote_tail_kernel<false>, dim3(pn2_ceil_div(n, 64), b), dim3(256), 0,
                     (hipStream_t)stream_, c, n, seed_features, net, seed_xyz, norm, vote_features,
                     vote_xyz, nullptr);
  return pn2_launch_status();
}

// d_net (b,3+c,n) whole, d_seed_features (b,c,n) and d_seed_xyz (b,n,3) (either may be NULL) from
// g_vote_xyz (b,n,3; NULL = zeros), g_vote_features (b,c,n) and the forward's vote_features and norm
PN2_API int votenet_vote_tail_grad(int b, int c, int n, const float *vote_features, const float *norm,
                                   const float *g_vote_xyz, const float *g_vote_features, float *d_net,
                                   float *d_seed_features, float *d_seed_xyz, void *stream_) {
  if (b <= 0 || c <= 0 || n <= 0) return 0;
  if (!vote_features || !norm || !g_vote_features || !d_net) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(vote_tail_kernel<true>, dim3(pn2_ceil_div(n, 64), b), dim3(256), 0,
                     (hipStream_t)stream_, c, n, vote_features, g_vote_features, g_vote_xyz,
                     const_cast<float *>(norm), d_net, d_seed_xyz, d_seed_features);
  return pn2_launch_status();
}

// x (b,c,n) -> y (b,c,n) = x / ||x||_2 over c, norm (b,n)
PN2_API int votenet_channel_normalize(int b, int c, int n, const float *x, float *y, float *norm,
                                      void *stream_) {
  if (b <= 0 || c <= 0 || n <= 0) return 0;
  hipLaunchKernelGGL(channel_normalize_kernel<false>, dim3(pn2_ceil_div(n, 64), b), dim3(256), 0,
                     (hipStream_t)stream_, c, n, x, nullptr, norm, y);
  return pn2_launch_status();
}

// dx (b,c,n) from dy, the forward's outputs y and norm
PN2_API int votenet_channel_normalize_grad(int b, int c, int n, const float *y, const float *norm,
                                           const float *dy, float *dx, void *stream_) {
  if (b <= 0 || c <= 0 || n <= 0) return 0;
  hipLaunchKernelGGL(channel_normalize_kernel<true>, dim3(pn2_ceil_div(n, 64), b), dim3(256), 0,
                     (hipStream_t)stream_, c, n, y, dy, const_cast<float *>(norm), dx);
  return pn2_launch_status();
}
