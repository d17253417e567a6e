// 3dioumatch_amd/csrc/common.h -- shared helpers for the gfx950 kernels.
//
// Arithmetic contract: fp32, source order, every operation rounded.
// All translation units are built with -ffp-contract=off AND the distance / geometry
// helpers below use the explicitly rounded intrinsics, so no a*b+c is ever fused.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>
#include <set>

#define PN2_API extern "C" __attribute__((visibility("default")))

constexpr int kWave = 64;  // CDNA wavefront width

static inline int pn2_launch_status() { return (int)hipGetLastError(); }

static inline int pn2_ceil_div(long long a, long long b) { return (int)((a + b - 1) / b); }

// XCD-aware block ids.  The dispatcher hands workgroup i (x fastest, then y, z) to XCD i % 8,
// and every XCD has a private 4 MB L2.  With the cloud index in the slowest grid dimension the
// default placement makes every XCD touch every cloud (each L2 re-fetches all of them); this
// remap gives each XCD a CONTIGUOUS range of logical block ids instead -- for B = 8 clouds
// exactly one cloud per XCD -- so a cloud's points / cell lists are fetched from HBM once and
// then hit in that XCD's L2.  Bijective for any grid size (cdna_hip_programming.md T1); purely
// a placement choice, no kernel depends on it for correctness.
struct BlockId { int x, y, z; };

__device__ __forceinline__ int xcd_contiguous_block(int hw, int nwg) {
  const int xcd = hw & 7, slot = hw >> 3, q = nwg >> 3, r = nwg & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
}

__device__ __forceinline__ BlockId xcd_block_id() {
  const int gx = gridDim.x, gy = gridDim.y;
  const int nwg = gx * gy * gridDim.z;
  int l = xcd_contiguous_block(blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z), nwg);
  BlockId o;
  o.x = l % gx;
  l /= gx;
  o.y = l % gy;
  o.z = l / gy;
  return o;
}

// Zero `bytes` (a multiple of 4) of device memory with an ordinary kernel.  Used instead of
// hipMemsetAsync so that, when the caller's stream is being captured into a HIP graph, the
// clear is a plain kernel node ordered like every other launch.
static __global__ void __launch_bounds__(256) pn2_zero_words_kernel(unsigned int *p, size_t words) {
  const size_t stride = (size_t)gridDim.x * 256 * 4;
  for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4; i < words; i += stride) {
    if (i + 4 <= words && ((size_t)(p + i) & 15) == 0) {
      *reinterpret_cast<uint4 *>(p + i) = make_uint4(0u, 0u, 0u, 0u);
    } else {
      for (size_t j = i; j < words && j < i + 4; ++j) p[j] = 0u;
    }
  }
}

static inline int pn2_zero_async(void *ptr, size_t bytes, hipStream_t stream) {
  const size_t words = bytes / 4;
  if (words == 0) return 0;
  long long blocks = (long long)((words + 1023) / 1024);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(pn2_zero_words_kernel, dim3((unsigned)blocks), dim3(256), 0, stream,
                     (unsigned int *)ptr, words);
  return (int)hipGetLastError();
}

// (ax-bx)^2 + (ay-by)^2 + (az-bz)^2, left to right, each op rounded to fp32.
// This is the expression every reference kernel uses for a squared distance
// (ball_query_gpu.cu:36-37, interpolate_gpu.cu:39, sampling_gpu.cu:108-109).
__device__ __forceinline__ float sqdist3(float ax, float ay, float az, float bx, float by,
                                         float bz) {
  const float dx = __fsub_rn(ax, bx), dy = __fsub_rn(ay, by), dz = __fsub_rn(az, bz);
  return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & (kWave - 1)); }

// number of set bits of `mask` strictly below this lane
__device__ __forceinline__ int mask_rank(unsigned long long mask) {
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32),
                                        __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// ---- wave reductions: butterflies in a FIXED order (summation order is part of the results) ------
// sum over the 64 lanes, every lane gets it; offsets 32, 16, .., 1
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = kWave / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

__device__ __forceinline__ double shfl_xor_f64(double v, int mask) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __shfl_xor(lo, mask, kWave);
  hi = __shfl_xor(hi, mask, kWave);
  return __hiloint2double(hi, lo);
}

// the same in double; offsets 1, 2, .., 32 (the other way round from the float form)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) v += shfl_xor_f64(v, off);
  return v;
}

// sum over the 32 lanes of each half-wave (DPP, no LDS); the total lands in lanes 16..31 / 48..63
__device__ __forceinline__ float half_wave_sum(float v) {
#define HW_STEP(CTRL, RM) v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, RM, 0xf, false))
  HW_STEP(0xB1, 0xf);   // quad_perm [1,0,3,2]
  HW_STEP(0x4E, 0xf);   // quad_perm [2,3,0,1]
  HW_STEP(0x141, 0xf);  // row_half_mirror
  HW_STEP(0x140, 0xf);  // row_mirror        -> every lane: the total of its row of 16
  HW_STEP(0x142, 0xa);  // row_bcast:15 into rows 1 and 3 -> the total of the half-wave
#undef HW_STEP
  return v;
}

// the same butterfly with max / min: lanes 16..31 (48..63) end up with the extreme of lanes
// 0..31 (32..63); masked-out rows keep their own value (old = v)
template <bool MAXOP>
__device__ __forceinline__ float half_wave_extreme(float v) {
#define HX_STEP(CTRL, RM)                                                                        \
  {                                                                                              \
    const float o = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(                      \
        __builtin_bit_cast(int, v), __builtin_bit_cast(int, v), CTRL, RM, 0xf, false));         \
    v = MAXOP ? fmaxf(v, o) : fminf(v, o);                                                       \
  }
  HX_STEP(0xB1, 0xf);
  HX_STEP(0x4E, 0xf);
  HX_STEP(0x141, 0xf);
  HX_STEP(0x140, 0xf);
  HX_STEP(0x142, 0xa);
#undef HX_STEP
  return v;
}

// ---- host side of the persistent / large-LDS launches ---------------------------------------------
// compute units of the current device (256 when it cannot be asked), asked once
static inline int pn2_cu_count() {
  static int cus = 0;
  if (!cus) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      cus = 256;
  }
  return cus;
}

// Let `kernel` be launched with up to `bytes` of dynamic LDS (above the 64 KB default): set once per
// kernel, remembered by address (the instantiations of a template share one pointer type), safe
// from several host threads.  The first call's `bytes` holds: pass the kernel's maximum.
static inline void pn2_allow_dynamic_lds(const void *kernel, size_t bytes) {
  static std::mutex mu;
  static std::set<const void *> done;
  std::lock_guard<std::mutex> lock(mu);
  if (done.insert(kernel).second)
    (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}
