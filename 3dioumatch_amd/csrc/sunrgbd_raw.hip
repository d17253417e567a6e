// 3dioumatch_amd/csrc/sunrgbd_raw.hip -- raw SUN RGB-D depth clouds -> the kept rows of the prepared
// layout and the store rows built from them (include/sunrgbd_raw_hip.h; votenet/sunrgbd_raw.py holds
// the readers, the box table, the host validation and the numpy restatement).  Every kernel is
// instantiated for float and double clouds: the arithmetic is the FILE's, rounded to float32 once.
//
//   sun_raw_gather_kernel  one thread per kept slot of the chunk.  The slot's scene is q / num_point
//                          (a workgroup, even a wave, may straddle two scenes); its raw row is the
//                          draw SB_DRAW_STUDENT of csrc/scene_common.h keyed by the scene's place in
//                          the whole export, or the given choice; the six values are copied.
//   sun_raw_floor_kernel   one workgroup per scene: np.percentile(kept z, 0.99); it also clears the
//                          scene's count of non-finite values.  The selection is the scheme
//                          of scan_prepare_kernel (csrc/scan_batch.hip) over the element type's key:
//                          8-bit radix passes from the top byte down (four for float32, eight for
//                          float64) find the key of rank lo, how many kept points share it and where
//                          lo falls among them; rank lo + 1 is the same key when it still falls among
//                          them and the smallest larger key (one more pass) otherwise.  Then numpy's
//                          lerp in the element type, every operation rounded, nothing fused.
//   sun_raw_rows_kernel    one thread per kept slot and per raw row, whichever are more.  The slot: x y
//                          z, r g b - 0.5 and z - floor in the element type, each rounded to float32
//                          once.  The raw row: its NaN and Inf values, counted over ALL raw rows of the
//                          scene (found by bisection of the offset table) with every compute unit
//                          reading, not one workgroup per scene; a wave without one -- every wave of a
//                          sound chunk -- issues nothing, the others one integer atomic per lane.
#include "common.h"
#include "scene_common.h"
#include "../../include/sunrgbd_raw_hip.h"

namespace {

constexpr int kBlock = 256;
constexpr int kFloorBlock = 1024;
constexpr int kFloorWaves = kFloorBlock / kWave;

// the scene whose raw rows hold row i: the largest s with off[s] <= i (every scene has a row)
__device__ __forceinline__ int find_scene(const long long *off, int S, long long i) {
  int lo = 0, hi = S - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= i) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// The element type's order-preserving key and its individually rounded arithmetic.
template <class T> struct Elem;

template <> struct Elem<float> {
  using Key = unsigned;
  static constexpr int kTopShift = 24;
  static constexpr Key kNone = 0xFFFFFFFFu;
  __device__ static __forceinline__ Key key(float v) { return order_key(v); }
  __device__ static __forceinline__ float value(Key k) { return from_order_key(k); }
  __device__ static __forceinline__ float add(float a, float b) { return __fadd_rn(a, b); }
  __device__ static __forceinline__ float sub(float a, float b) { return __fsub_rn(a, b); }
  __device__ static __forceinline__ float mul(float a, float b) { return __fmul_rn(a, b); }
  __device__ static __forceinline__ float quantile() { return 0.99f / 100.0f; }  // f32(0.99) / f32(100)
};

template <> struct Elem<double> {
  using Key = unsigned long long;
  static constexpr int kTopShift = 56;
  static constexpr Key kNone = 0xFFFFFFFFFFFFFFFFull;
  __device__ static __forceinline__ Key key(double v) {
    const Key u = (Key)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
  }
  __device__ static __forceinline__ double value(Key k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
  }
  __device__ static __forceinline__ double add(double a, double b) { return __dadd_rn(a, b); }
  __device__ static __forceinline__ double sub(double a, double b) { return __dsub_rn(a, b); }
  __device__ static __forceinline__ double mul(double a, double b) { return __dmul_rn(a, b); }
  __device__ static __forceinline__ double quantile() { return 0.99 / 100.0; }
};

template <class T>
__global__ void __launch_bounds__(kBlock) sun_raw_gather_kernel(const SunRgbdRawArgs a) {
  const long long q = (long long)blockIdx.x * kBlock + threadIdx.x;
  const int N = a.num_point;
  if (q >= (long long)a.S * N) return;
  const int s = (int)(q / N), j = (int)(q - (long long)s * N);
  const long long first = a.raw_offset[s];
  const int n = (int)(a.raw_offset[s + 1] - first);  // 1 <= n < 2^30: the host's check
  int p;
  if (a.keep[s] == SUNRAW_KEEP_GIVEN) {
    p = a.choice[q];  // 0 <= p < n: the host's check
  } else {
    const unsigned key = draw_key(a.seed, 0u, (unsigned)a.scan_index[s], SB_DRAW_STUDENT);
    p = sample_index(key, j, n, N, feistel_half_bits(n));
  }
  const T *src = (const T *)a.raw + (size_t)(first + p) * 6;
  T *dst = (T *)a.kept + (size_t)q * 6;
#pragma unroll
  for (int c = 0; c < 6; ++c) dst[c] = src[c];
}

template <class T>
__global__ void __launch_bounds__(kFloorBlock) sun_raw_floor_kernel(const SunRgbdRawArgs a) {
  using E = Elem<T>;
  using Key = typename E::Key;
  __shared__ unsigned s_hist[kFloorWaves * 256];  // one histogram per wave: less contention
  __shared__ unsigned s_tot[256];
  __shared__ Key s_prefix, s_next;
  __shared__ unsigned s_rank, s_equal;
  const int scene = blockIdx.x, t = threadIdx.x, wave = t / kWave;
  const int n = a.num_point;
  const T *z = (const T *)a.kept + (size_t)scene * n * 6 + 2;  // kept z of slot i: z[i * 6]
  if (t == 0) s_next = E::kNone;  // (read behind the barriers of the passes below)

  // numpy's virtual index of the linear method in the element type: (n - 1) * (0.99 / 100)
  const T v = E::mul(E::quantile(), (T)(n - 1));
  const int lo = min((int)floor(v), n - 1);
  const int hi = min(lo + 1, n - 1);
  const T g = E::sub(v, (T)lo);

  Key prefix = 0, mask = 0;
  unsigned rank = (unsigned)lo;
  for (int shift = E::kTopShift; shift >= 0; shift -= 8) {
    for (int i = t; i < kFloorWaves * 256; i += kFloorBlock) s_hist[i] = 0u;
    __syncthreads();
    for (int i = t; i < n; i += kFloorBlock) {
      const Key key = E::key(z[(size_t)i * 6]);
      if ((key & mask) == prefix) atomicAdd(&s_hist[wave * 256 + (int)((key >> shift) & 255u)], 1u);
    }
    __syncthreads();
    if (t < 256) {
      unsigned s = 0u;
      for (int w = 0; w < kFloorWaves; ++w) s += s_hist[w * 256 + t];
      s_tot[t] = s;
    }
    __syncthreads();
    if (t == 0) {
      unsigned cum = 0u;
      int d = 0;
      for (; d < 255; ++d) {
        if (rank < cum + s_tot[d]) break;
        cum += s_tot[d];
      }
      s_prefix = prefix | ((Key)d << shift);
      s_rank = rank - cum;
      s_equal = s_tot[d];
    }
    __syncthreads();
    prefix = s_prefix;
    rank = s_rank;
    mask |= (Key)255u << shift;
  }
  // prefix: the key of rank lo; s_equal kept points share it and lo is number `rank` of them
  const bool same = hi == lo || rank + 1u < s_equal;
  if (!same) {
    Key next = E::kNone;
    for (int i = t; i < n; i += kFloorBlock) {
      const Key key = E::key(z[(size_t)i * 6]);
      if (key > prefix && key < next) next = key;
    }
    if (next != E::kNone) atomicMin(&s_next, next);
  }
  __syncthreads();
  if (t != 0) return;
  const T lower = E::value(prefix);
  const T upper = (same || s_next == E::kNone) ? lower : E::value(s_next);
  // numpy.lib._function_base_impl._lerp: a + (b - a) t, and b - (b - a)(1 - t) where t >= 0.5
  const T diff = E::sub(upper, lower);
  ((T *)a.floor)[scene] = g >= (T)0.5 ? E::sub(upper, E::mul(diff, E::sub((T)1, g)))
                                      : E::add(lower, E::mul(diff, g));
  a.nonfinite[scene] = 0ull;  // sun_raw_rows_kernel, the next launch, counts into it
}

template <class T>
__global__ void __launch_bounds__(kBlock) sun_raw_rows_kernel(const SunRgbdRawArgs a) {
  using E = Elem<T>;
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  const int N = a.num_point;
  if (i < (long long)a.S * N) {  // kept slot i
    const T floor = ((const T *)a.floor)[(int)(i / N)];
    const T *k = (const T *)a.kept + (size_t)i * 6;
    float *out = a.rows + (size_t)i * SUNRAW_ROW_COLS;
    const T x = k[0], y = k[1], z = k[2];
    out[0] = (float)x;
    out[1] = (float)y;
    out[2] = (float)z;
#pragma unroll
    for (int c = 3; c < 6; ++c) out[c] = (float)E::sub(k[c], (T)0.5);  // rgb - MEAN_COLOR_RGB
    out[6] = (float)E::sub(z, floor);
  }
  unsigned bad = 0u;
  if (i < a.P) {  // raw row i
    const T *r = (const T *)a.raw + (size_t)i * 6;
#pragma unroll
    for (int c = 0; c < 6; ++c) bad += isfinite(r[c]) ? 0u : 1u;
  }
  if (__ballot(bad != 0u) == 0ull) return;
  if (bad) atomicAdd(&a.nonfinite[find_scene(a.raw_offset, a.S, i)], (unsigned long long)bad);
}

template <class T>
int export_chunk(const SunRgbdRawArgs &a, hipStream_t st) {
  const long long Q = (long long)a.S * a.num_point;
  hipLaunchKernelGGL(sun_raw_gather_kernel<T>, dim3(pn2_ceil_div(Q, kBlock)), dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL(sun_raw_floor_kernel<T>, dim3(a.S), dim3(kFloorBlock), 0, st, a);
  hipLaunchKernelGGL(sun_raw_rows_kernel<T>, dim3(pn2_ceil_div(Q > a.P ? Q : a.P, kBlock)), dim3(kBlock), 0, st, a);
  return (int)hipGetLastError();
}

}  // namespace

PN2_API int scene_sunrgbd_raw_export(const SunRgbdRawArgs *args, void *stream) {
  const long long limit = 0x7FFFFFFFll;
  if (!args || args->S < 1 || args->num_point < 1 || (long long)args->S * args->num_point > limit ||
      args->P < args->S || args->P > limit || (args->elem != SUNRAW_FLOAT32 && args->elem != SUNRAW_FLOAT64) ||
      !args->raw || !args->raw_offset || !args->keep || !args->scan_index || !args->choice || !args->kept || !args->floor ||
      !args->nonfinite || !args->rows)
    return (int)hipErrorInvalidValue;
  return args->elem == SUNRAW_FLOAT64 ? export_chunk<double>(*args, (hipStream_t)stream)
                                      : export_chunk<float>(*args, (hipStream_t)stream);
}
