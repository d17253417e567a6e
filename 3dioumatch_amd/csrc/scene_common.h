// 3dioumatch_amd/csrc/scene_common.h -- what the batch builders share (scene_batch.hip for ScanNet,
// sunrgbd_batch.hip for SUN RGB-D, scan_batch.hip for scans without labels): the counter-based draw
// hash and the point sampler.  The host form of every function here is in votenet/scene_loader.py
// (mix32, draw_key, _element, _feistel, sample_indices), which all three loaders import; a change
// here changes every batch of every loader.
#pragma once
#include "common.h"

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
