// 3dioumatch_amd/csrc/mlp_frag.h -- everything a lane does with a bf16 MFMA fragment, once: the exact
// three-term split of fp32 values, the six-MFMA product, the fragment-ordered weight images and
// their reads, the transposing LDS read, and the LIN4 image layout that mlp_chain.hip writes and
// mlp_eval_pool.hip reads.  Included through mlp_operand.h by every mlp_* translation unit; whatever
// changes a fragment's arithmetic or the LIN4 image layout belongs here and nowhere else.
#pragma once
#include "common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- fp32 products on the bf16 matrix pipe -----------------------------------------------------
// v_mfma_f32_32x32x2_f32 runs at 1/16 of the bf16 rate.  An fp32 value is the EXACT sum of three
// bf16 values (truncation split: hi = the top 8 significand bits, mid = the next 8, lo = the
// last 8; each difference is exact), a bf16 x bf16 product is exact in fp32, and the matrix pipe
// accumulates in fp32.  Of the nine partial products of a * b the three below 2^-24 |a b|
// (mid*lo, lo*mid, lo*lo) are dropped -- the same order as one fp32 rounding -- and the other six
// are issued as v_mfma_f32_32x32x16_bf16: 6 x 32 cycles per 16 k instead of 8 x 64 (2.7x less
// matrix time) for fp32-grade results (max error over the layer shapes 1e-7 of the output
// range, profiles/r4_split_bf16.json).  A lane's MFMA operand (row / column lane & 31, k half
// lane >> 5, eight consecutive k) is exactly what the k-quad LDS layout hands it in two 16-byte
// reads, so the split happens on the fragments, in registers.
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef short bf16x4 __attribute__((ext_vector_type(4)));
struct Split3 { bf16x8 hi, mid, lo; };

__device__ __forceinline__ unsigned pack_hi16(float a, float b) {  // (b.hi16 << 16) | a.hi16
  return __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, b), __builtin_bit_cast(unsigned, a), 0x07060302u);
}

// one step of the split: x = top + rest exactly, top = x truncated to bf16 (held as a float)
__device__ __forceinline__ void split_top(float x, float &top, float &rest) {
  top = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, x) & 0xffff0000u);
  rest = x - top;
}

// x = h + m + l exactly, each term a bf16 value held as a float; l has at most 8 significant bits
__device__ __forceinline__ void split_terms(float x, float &h, float &m, float &l) {
  float r1;
  split_top(x, h, r1);
  split_top(r1, m, l);
}

__device__ __forceinline__ Split3 split3(const float4 &u, const float4 &v) {
  const float x[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
  float h[8], m[8], l[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) split_terms(x[e], h[e], m[e], l[e]);
  typedef unsigned u32x4v __attribute__((ext_vector_type(4)));
  u32x4v ph, pm, pl;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    ph[e] = pack_hi16(h[2 * e], h[2 * e + 1]);
    pm[e] = pack_hi16(m[2 * e], m[2 * e + 1]);
    pl[e] = pack_hi16(l[2 * e], l[2 * e + 1]);
  }
  Split3 o;
  o.hi = __builtin_bit_cast(bf16x8, ph);
  o.mid = __builtin_bit_cast(bf16x8, pm);
  o.lo = __builtin_bit_cast(bf16x8, pl);
  return o;
}

// the same split of eight values given one by one (fragments gathered with 4-byte LDS reads)
__device__ __forceinline__ Split3 split3(const float (&x)[8]) {
  return split3(make_float4(x[0], x[1], x[2], x[3]), make_float4(x[4], x[5], x[6], x[7]));
}

// the terms of four consecutive columns (from c0) of row `row` -> a row-major bf16 image with RP
// bytes per row: 8 bytes per term, the terms' images term_bytes apart
template <int RP>
__device__ __forceinline__ void store_terms4(char *img, size_t term_bytes, int row, int c0, const float (&h)[4],
                                             const float (&m)[4], const float (&l)[4]) {
  char *dst = img + (size_t)row * RP + c0 * 2;
  *reinterpret_cast<uint2 *>(dst) = make_uint2(pack_hi16(h[0], h[1]), pack_hi16(h[2], h[3]));
  *reinterpret_cast<uint2 *>(dst + term_bytes) = make_uint2(pack_hi16(m[0], m[1]), pack_hi16(m[2], m[3]));
  *reinterpret_cast<uint2 *>(dst + 2 * term_bytes) = make_uint2(pack_hi16(l[0], l[1]), pack_hi16(l[2], l[3]));
}

// four values split and stored
template <int RP>
__device__ __forceinline__ void store_split4(char *img, size_t term_bytes, int row, int c0, const float (&v)[4]) {
  float h[4], m[4], l[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) split_terms(v[e], h[e], m[e], l[e]);
  store_terms4<RP>(img, term_bytes, row, c0, h, m, l);
}

// acc += a * b over the lane group's 16 k, fp32-grade: the six significant partial products,
// small ones first
__device__ __forceinline__ void mfma_x6(f32x16 &acc, const Split3 &a, const Split3 &b) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.lo, b.hi, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.hi, b.lo, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.mid, b.mid, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.mid, b.hi, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.hi, b.mid, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.hi, b.hi, acc, 0, 0, 0);
}

// ds_read_b64_tr_b16: the 16 lanes of a group hand in the addresses of a 4 x 16 block of a row-major
// bf16 image as sixteen 8-byte pieces and receive its transpose (mlp_bwd_x6.h says which lane gets what)
__device__ __forceinline__ bf16x4 lds_read_tr(const char *p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) bf16x4 *)(__attribute__((address_space(3))) char *)p);
}

// ---- fragment-ordered weight images --------------------------------------------------------------
// byte offset of fragment (term, step t, half h, row) in a K-deep weight image of R rows
template <int K, int R>
__device__ __forceinline__ int img_off(int term, int t, int h, int row) {
  return (((term * (K / 16) + t) * 2 + h) * R + row) * 16;
}

__device__ __forceinline__ Split3 lds_frag(const char *p, int term_stride) {
  Split3 s;
  s.hi = *reinterpret_cast<const bf16x8 *>(p);
  s.mid = *reinterpret_cast<const bf16x8 *>(p + term_stride);
  s.lo = *reinterpret_cast<const bf16x8 *>(p + 2 * term_stride);
  return s;
}

__device__ __forceinline__ void store_frag(char *dst, int term_stride, const Split3 &s) {
  *reinterpret_cast<bf16x8 *>(dst) = s.hi;
  *reinterpret_cast<bf16x8 *>(dst + term_stride) = s.mid;
  *reinterpret_cast<bf16x8 *>(dst + 2 * term_stride) = s.lo;
}

// acc[i] += w[i] x s (N form: the weight is the A operand) or s x w[i] (T form), i < NB: the six
// significant partial products, small ones first, the NB independent accumulators interleaved
// (the forms: mlp_chain.hip's header comment)
template <int NB, bool TFORM, bool FIRST = false>
__device__ __forceinline__ void mfma6(f32x16 (&acc)[NB], const Split3 &s, const Split3 (&w)[NB]) {
  // FIRST: the accumulators are not read -- the first product starts from a literal zero (an inline
  // constant of the MFMA: no register is cleared; 96 v_mov per tile otherwise)
  const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#define FRAG_STEP(WT, ST, C0)                                                                      \
  _Pragma("unroll") for (int i = 0; i < NB; ++i)                                                  \
    acc[i] = TFORM ? __builtin_amdgcn_mfma_f32_32x32x16_bf16(s.ST, w[i].WT, (C0) ? zero : acc[i], 0, 0, 0) \
                   : __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[i].WT, s.ST, (C0) ? zero : acc[i], 0, 0, 0)
  FRAG_STEP(lo, hi, FIRST);
  FRAG_STEP(hi, lo, false);
  FRAG_STEP(mid, mid, false);
  FRAG_STEP(mid, hi, false);
  FRAG_STEP(hi, mid, false);
  FRAG_STEP(hi, hi, false);
#undef FRAG_STEP
}

// ---- the LIN4 image (SA1, 4 -> 64 -> 64 -> 128): what mlp_chain_lin4_prepare leaves in global
// memory and both the training chain (mlp_chain.hip) and the eval pass (mlp_eval_pool.hip) copy
// into LDS: [64 x 64 image, N form][128 x 64 image, T form][first-layer rows (float4)][(sc, sh) of
// the first layer's BatchNorm (float2)].  An image is 3 terms x rows x K x 2 bytes.
constexpr int kLin4K = 64;                                      // channels entering the two MFMA layers
constexpr int kLin4ImgA = 3 * (kLin4K / 16) * 2 * 64 * 16;      // 24 576
constexpr int kLin4ImgB = 3 * (kLin4K / 16) * 2 * 128 * 16;     // 49 152
constexpr int kLin4TabW = kLin4ImgA + kLin4ImgB;                // offset of the first layer's rows
constexpr int kLin4TabC = kLin4TabW + 64 * 16;                  // offset of its (sc, sh) pairs
constexpr int kLin4TabBytes = 64 * 16 + 64 * 8;
constexpr int kLin4ImgBytes = kLin4TabW + kLin4TabBytes;        // 75 264

}  // namespace
