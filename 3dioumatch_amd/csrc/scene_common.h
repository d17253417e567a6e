// 3dioumatch_amd/csrc/scene_common.h -- the device core of the batch builders (scene_batch.hip for
// ScanNet, sunrgbd_batch.hip for SUN RGB-D, scan_batch.hip for scans without labels): the
// counter-based draw hash, the point sampler, a row's augmentation draws (RowAug), the row header
// they are written to, the float32-staged transform of a point, the float64 transform of a label
// vector and the order-preserving integer keys of a float.  Anything that changes a row's arithmetic
// belongs here: the builders call these functions and restate none of them, so a change here changes
// every batch of every loader.  The host forms are in votenet/scene_loader.py (mix32, draw_key,
// _element, _feistel, sample_indices), which all three loaders import, and in each dataset's module
// (host_draws, host_scene), which stay independent of this file: they are the yardstick.
#pragma once
#include "common.h"
#include "../../include/scene_hip.h"    // SB_DRAW_FLIP_X
#include "../../include/sunrgbd_hip.h"  // SUN_DRAW_FLIP

__device__ __forceinline__ unsigned mix32(unsigned h) {  // murmur3 finaliser
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

// key of (seed, counter, row, draw): every random quantity of a batch derives from one of these
__device__ __forceinline__ unsigned draw_key(unsigned seed, unsigned counter, unsigned row,
                                             unsigned draw) {
  unsigned h = mix32(seed * 0x9E3779B9u + 0x85EBCA6Bu);
  h = mix32(h ^ (counter * 0xC2B2AE35u + 0x27D4EB2Fu));
  h = mix32(h ^ (row * 0x165667B1u + 0xD3A2646Cu));
  return mix32(h ^ (draw * 0xFD7046C5u + 0xB55A4F09u));
}

__device__ __forceinline__ unsigned element(unsigned key, unsigned j) {
  return mix32(key ^ (j * 0x9E3779B9u + 0x7F4A7C15u));
}

// 4-round balanced Feistel network on 2h bits: a bijection of [0, 4^h)
__device__ __forceinline__ unsigned feistel(unsigned x, int h, unsigned key) {
  const unsigned mask = (1u << h) - 1u;
  unsigned l = x >> h, r = x & mask;
  for (unsigned round = 0; round < 4; ++round) {
    const unsigned f = mix32(r ^ element(key, round)) & mask;
    const unsigned nl = r;
    r = l ^ f;
    l = nl;
  }
  return (l << h) | r;
}

__device__ __forceinline__ int feistel_half_bits(int n) {  // smallest h with 4^h >= n, h >= 1
  int h = 1;  // n < 2^30 (checked at load)
  while (h < 15 && (1u << (2 * h)) < (unsigned)n) ++h;
  return h;
}

// slot j of a draw of N of n points: distinct for n >= N (slots 0..N-1 of the cycle-walked
// bijection), i.i.d. with replacement otherwise (pc_util.random_sampling: replace = n < N)
__device__ __forceinline__ int sample_index(unsigned key, int j, int n, int N, int h) {
  if (n < N) return (int)(((unsigned long long)element(key, (unsigned)j) * (unsigned)n) >> 32);
  unsigned x = feistel((unsigned)j, h, key);
  while (x >= (unsigned)n) x = feistel(x, h, key);
  return (int)x;
}

// monotone integer image of a float: a < b <=> order_key(a) < order_key(b)
__device__ __forceinline__ unsigned order_key(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float from_order_key(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// A row's augmentation: flips, the rotation about z (cos, sin, angle) and the isotropic scale.
struct RowAug {
  int fx, fy;
  double c, s, angle, scale;
};

// the row that is not augmented (eval rows, teacher samples)
__device__ __forceinline__ RowAug row_identity() { return RowAug{0, 0, 1.0, 0.0, 0.0, 1.0}; }

// The draws of batch row `row`.  ScanNet: four uniforms (flip x, flip y, angle, scale), +-5 degree;
// SUN RGB-D (`sun`): three (flip, angle, scale), +-30 degree, no y flip.  `u_in` (NULL: drawn here)
// holds explicit uniforms, row `u_row` of it is this row's -- the unlabeled rows' launch indexes its
// own array by r and keys the draw by row0 + r.
__device__ __forceinline__ RowAug row_aug(bool sun, const double *u_in, int u_row, unsigned seed,
                                          unsigned counter, unsigned row) {
  const int nu = sun ? 3 : 4;
  const unsigned first = sun ? (unsigned)SUN_DRAW_FLIP : (unsigned)SB_DRAW_FLIP_X;
  auto u = [&](int k) {
    return u_in ? u_in[u_row * nu + k] : (double)draw_key(seed, counter, row, first + k) * 0x1p-32;
  };
  RowAug g;
  g.fx = u(0) > 0.5;
  if (sun) {
    g.fy = 0;
    g.angle = (u(1) * M_PI) / 3.0 - M_PI / 6.0;  // -30 ~ +30 degree
    g.scale = u(2) * 0.3 + 0.85;
  } else {
    g.fy = u(1) > 0.5;
    g.angle = (u(2) * M_PI) / 18.0 - M_PI / 36.0;  // -5 ~ +5 degree
    g.scale = u(3) * 0.3 + 0.85;
  }
  g.c = cos(g.angle);
  g.s = sin(g.angle);
  return g;
}

// flip_x_axis, flip_y_axis, rot_angle, rot_mat and scale of row `row` in any of the three argument
// records; NULL flip_x_axis: no header asked for.  For row_identity() m[1] is (float)-0.0: the word
// of -0.0f, as the reference's rotz(0) negates a zero.
template <class Args>
__device__ __forceinline__ void write_row_header(const Args &a, int row, const RowAug &g) {
  if (!a.flip_x_axis) return;
  a.flip_x_axis[row] = g.fx;
  a.flip_y_axis[row] = g.fy;
  a.rot_angle[row] = (float)g.angle;
  float *m = a.rot_mat + row * 9;
  m[0] = (float)g.c; m[1] = (float)-g.s; m[2] = 0.0f;
  m[3] = (float)g.s; m[4] = (float)g.c;  m[5] = 0.0f;
  m[6] = 0.0f;       m[7] = 0.0f;        m[8] = 1.0f;
  const float sc = (float)g.scale;
  a.scale[row * 3 + 0] = sc;
  a.scale[row * 3 + 1] = sc;
  a.scale[row * 3 + 2] = sc;
}

// The scale stage of a float32 channel (a rotated coordinate, the height): float64, rounded once.
__device__ __forceinline__ float aug_scale(const RowAug &g, float v) {
  return (float)((double)v * g.scale);
}

// A point of the student's float32 cloud: flip, rotate, scale, each stage in float64 and rounded to
// float32 as the reference's float32 cloud is.  The `* 0.0` terms and their order are numpy's dot
// with the full rotation matrix: part of the rounding contract.
__device__ __forceinline__ void aug_point(const RowAug &g, float &x, float &y, float &z) {
  if (g.fx) x = -x;
  if (g.fy) y = -y;
  const double dx = x, dy = y, dz = z;
  const float rx = (float)(dx * g.c + dy * -g.s + dz * 0.0);
  const float ry = (float)(dx * g.s + dy * g.c + dz * 0.0);
  const float rz = (float)(dx * 0.0 + dy * 0.0 + dz * 1.0);
  x = aug_scale(g, rx);
  y = aug_scale(g, ry);
  z = aug_scale(g, rz);
}

// A float64 label vector (a box centre, a vote): flip, rotate, scale with no rounding in between.
__device__ __forceinline__ void aug_vector(const RowAug &g, double &x, double &y, double &z) {
  if (g.fx) x = -1.0 * x;
  if (g.fy) y = -1.0 * y;
  const double rx = x * g.c + y * -g.s + z * 0.0;
  const double ry = x * g.s + y * g.c + z * 0.0;
  const double rz = x * 0.0 + y * 0.0 + z * 1.0;
  x = rx * g.scale;
  y = ry * g.scale;
  z = rz * g.scale;
}
