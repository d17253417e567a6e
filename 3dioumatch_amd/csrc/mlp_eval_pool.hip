// 3dioumatch_amd/csrc/mlp_eval_pool.hip -- the pooled shared MLP of a set-abstraction level in EVAL
// mode as ONE pass: conv(1x1) -> BN -> ReLU -> conv -> BN -> ReLU -> conv -> BN -> ReLU -> max over
// nsample (pointnet2/pytorch_utils.py:14-39,70-124 + pointnet2_modules.py:256-262) with every
// BatchNorm a fixed per-channel affine (scale, shift) folded from the running statistics
// (mlp_bn_eval_coeff).  No intermediate activation is written: the only store is the pooled
// (B, C_out, m).
//
// In training mode this fusion is impossible (a layer's BatchNorm needs the statistics of ALL of
// its output before any of it can be activated); in eval mode it is straightforward.
// The MFMA forms are those of mlp_chain.hip (its header comment): a layer in N form leaves its
// activation in registers as the next layer's operand, the last layer runs in T form so that
// BatchNorm + ReLU + the max over nsample are in-lane.  Every fp32 product is six bf16 MFMAs on
// the exact three-term split (mlp_frag.h).
//
// Two input forms:
//   LIN4 (SA1, 4 -> 64 -> 64 -> 128): layer 0 recomputed per element from the 4-channel grouped
//        input (lin4), layer 1 in N form, layer 2 in T form.  Weight images: mlp_chain_lin4_prepare
//        (72 KB in LDS, two workgroups per CU).
//   STORED (SA2 - SA4, vote aggregation, IoU branch; 128 -> 128 -> C_out, C_out 128 / 256): the
//        input is layer 0's raw output, its BatchNorm + ReLU applied at load.  The three-term images
//        of W1 (128 x 128, 96 KB) and W2 (C_out x 128, up to 192 KB) do not both fit the 160 KB of
//        LDS: W1's image is in LDS (every fragment read by all four waves of every tile, in N form
//        the operand whose reads a wave cannot share), W2's fragments come from L2 (one coalesced
//        16-byte read per lane, term and block: the image is 96 / 192 KB, resident in every XCD's
//        L2).  Recomputing layer 1 per half of C_out would still need 96 + 96 KB: no layout with
//        both images in LDS exists at 256 outputs.
#include "common.h"
#include "mlp_operand.h"

namespace {

// relu(bn(.)) of eight N-form accumulator registers (block t >> 1, registers 8 (t & 1) + e), the
// k slots of step t of the next (T-form) layer: channel 16 t + 8 (e >> 2) + 4 h + (e & 3)
template <int NB>
__device__ __forceinline__ Split3 ev_act_of_acc(const f32x16 (&acc)[NB], int t, const float2 *ch) {
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float2 c = ch[16 * t + 8 * (e >> 2) + (e & 3)];
    v[e] = fmaxf(__fmaf_rn(acc[t >> 1][8 * (t & 1) + e], c.x, c.y), 0.f);
  }
  return split3(v);
}

// Pooled epilogue of NB T-form blocks (lane = channel 32 (j0 + j) + l31, register q = sample
// (q & 3) + 8 (q >> 2) + 4 h of the tile): best = max over the group of bn(y); relu(max) = max(relu).
// NS == 16: two groups per tile; NS == 32: one; NS == 64: one group over two consecutive tiles
// (p = 0, 1), `best` carried between them.
template <int NB, int NS>
__device__ __forceinline__ void ev_pool(const f32x16 (&acc)[NB], const float2 *c_out, int j0, int l31,
                                        float (&best)[NB][2], int p) {
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const float2 c = c_out[32 * (j0 + j) + l31];
    if (p == 0) { best[j][0] = -__builtin_inff(); best[j][1] = -__builtin_inff(); }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int gq = NS == 16 ? (q >> 3) : 0;
      best[j][gq] = fmaxf(best[j][gq], __fmaf_rn(acc[j][q], c.x, c.y));
    }
  }
}

// the two half-waves hold different samples of the same channel: combine, relu, store (h == 0)
template <int NB, int NS>
__device__ __forceinline__ void ev_pool_store(float (&best)[NB][2], float *out, size_t row0, int groups,
                                              int g0, int l31, int h) {
#pragma unroll
  for (int j = 0; j < NB; ++j)
#pragma unroll
    for (int gq = 0; gq < (NS == 16 ? 2 : 1); ++gq) {
      const float o = fmaxf(fmaxf(best[j][gq], __shfl_xor(best[j][gq], 32, kWave)), 0.f);
      if (h == 0) out[(row0 + 32 * j + l31) * groups + g0 + gq] = o;
    }
}

// ================================ LIN4 form (SA1) ===============================================
// the image [W1][W2T][w0 rows (float4)][(sc0, sh0)]: mlp_frag.h (kLin4*)
constexpr int kL4Lds = kLin4ImgBytes + 64 * 8 + 128 * 8;   // + (sc1, sh1) + (sc2, sh2)
constexpr int kL4TilesPerWave = 2;

struct Lin4Args {
  int r;                 // columns per cloud (m * ns)
  int tiles_per_cloud;   // r / 32
  const float *x4;       // (b, 4, r)
  const char *wimg;      // mlp_chain_lin4_prepare's image (w0, sc0, sh0, w1, w2)
  const float *sc1, *sh1, *sc2, *sh2;
  float *out;            // (b, 128, r / NS)
};

template <int NS>
__global__ void __launch_bounds__(256, 2) eval_lin4_kernel(const Lin4Args a) {
  constexpr int M1 = 64, M2 = 128, M2B = 4, T = kLin4K / 16;
  constexpr int W1_TERM = kLin4ImgA / 3, W2_TERM = kLin4ImgB / 3;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  char *w1img = lds, *w2img = lds + kLin4ImgA;
  float4 *w0tab = reinterpret_cast<float4 *>(lds + kLin4TabW);
  float2 *c0tab = reinterpret_cast<float2 *>(lds + kLin4TabC);
  float2 *c1tab = reinterpret_cast<float2 *>(lds + kLin4ImgBytes);
  float2 *c2tab = reinterpret_cast<float2 *>(lds + kLin4ImgBytes + 64 * 8);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  {
    const uint4 *src = reinterpret_cast<const uint4 *>(a.wimg);
    uint4 *dst = reinterpret_cast<uint4 *>(lds);
    for (int i = tid; i < kLin4ImgBytes / 16; i += 256) dst[i] = src[i];
    if (tid < 64) c1tab[tid] = make_float2(a.sc1[tid], a.sh1[tid]);
    if (tid < 128) c2tab[tid] = make_float2(a.sc2[tid], a.sh2[tid]);
  }
  __syncthreads();

  const float4 *w0h = w0tab + 8 * h;
  const float2 *c0h = c0tab + 8 * h;
  const float2 *c1h = c1tab + 4 * h;
  const char *w1lane = w1img + (h * M1 + l31) * 16;
  const char *w2lane = w2img + (h * M2 + l31) * 16;
  constexpr int TPG = NS > 32 ? NS / 32 : 1;
  float best[M2B][2];

  auto load_x = [&](int tile, float (&x)[4]) {
    const int b = tile / a.tiles_per_cloud, col = (tile - b * a.tiles_per_cloud) * 32 + l31;
    const float *p = a.x4 + (size_t)b * 4 * a.r + col;
#pragma unroll
    for (int c = 0; c < 4; ++c) x[c] = p[(size_t)c * a.r];
  };
  const int tile0 = ((int)blockIdx.x * 4 + wave) * kL4TilesPerWave;
  float xn[4];
  load_x(tile0, xn);
#pragma unroll 1
  for (int it = 0; it < kL4TilesPerWave; ++it) {
    const int tile = tile0 + it;
    const int b = tile / a.tiles_per_cloud, col0 = (tile - b * a.tiles_per_cloud) * 32;
    float x[4] = {xn[0], xn[1], xn[2], xn[3]};
    if (it + 1 < kL4TilesPerWave) load_x(tile + 1, xn);

    // ---- layer 1 (N form) over the 64 recomputed channels of layer 0
    f32x16 acc1[2];
    auto prep0 = [&](int t) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float4 w = w0h[16 * t + e];
        const float2 c = c0h[16 * t + e];
        v[e] = fmaxf(__fmaf_rn(lin4(w, x[0], x[1], x[2], x[3]), c.x, c.y), 0.f);
      }
      return split3(v);
    };
    auto load_w1 = [&](int t, Split3 (&w)[2]) {
#pragma unroll
      for (int i = 0; i < 2; ++i) w[i] = lds_frag(w1lane + img_off<kLin4K, M1>(0, t, 0, 32 * i), W1_TERM);
    };
    {
      Split3 sc = prep0(0), wc[2];
      load_w1(0, wc);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 0; t < T; ++t) {
        Split3 sn = sc, wn[2] = {wc[0], wc[1]};
        if (t + 1 < T) {
          sn = prep0(t + 1);
          load_w1(t + 1, wn);
        }
        if (t == 0) mfma6<2, false, true>(acc1, sc, wc);
        else mfma6<2, false>(acc1, sc, wc);
        sc = sn; wc[0] = wn[0]; wc[1] = wn[1];
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // ---- layer 2 (T form) on relu(bn(acc1)), the four channel blocks in two halves
    f32x16 acc2[M2B];
    auto load_w2 = [&](int t, int j0, Split3 (&w)[2]) {
#pragma unroll
      for (int i = 0; i < 2; ++i) w[i] = lds_frag(w2lane + img_off<kLin4K, M2>(0, t, 0, 32 * (j0 + i)), W2_TERM);
    };
    {
      f32x16 lo2[2], hi2[2];
      Split3 sc = ev_act_of_acc(acc1, 0, c1h), wa[2], wb[2];
      load_w2(0, 0, wa);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 0; t < T; ++t) {
        load_w2(t, 2, wb);
        Split3 sn = sc;
        if (t + 1 < T) sn = ev_act_of_acc(acc1, t + 1, c1h);
        if (t == 0) mfma6<2, true, true>(lo2, sc, wa);
        else mfma6<2, true>(lo2, sc, wa);
        __builtin_amdgcn_sched_barrier(0);
        if (t + 1 < T) load_w2(t + 1, 0, wa);
        if (t == 0) mfma6<2, true, true>(hi2, sc, wb);
        else mfma6<2, true>(hi2, sc, wb);
        sc = sn;
        __builtin_amdgcn_sched_barrier(0);
      }
      acc2[0] = lo2[0]; acc2[1] = lo2[1]; acc2[2] = hi2[0]; acc2[3] = hi2[1];
    }
    const int p = it % TPG;
    ev_pool<M2B, NS>(acc2, c2tab, 0, l31, best, p);
    if (p == TPG - 1) {
      const int groups = a.r / NS;
      const int g0 = NS == 16 ? col0 / 16 : (col0 - 32 * p) / NS;
      ev_pool_store<M2B, NS>(best, a.out, (size_t)b * M2, groups, g0, l31, h);
    }
  }
}

bool lin4_shape_ok(int b, int m, int ns) {
  if (b <= 0 || m <= 0 || !(ns == 16 || ns == 32 || ns == 64)) return false;
  const long long r = (long long)m * ns;
  return r % (32 * 4 * kL4TilesPerWave) == 0 && (long long)b * r < (1LL << 31);
}

// ================================ STORED form (128 -> 128 -> C_out) =============================
constexpr int kStK = 128;                                   // channels entering layers 1 and 2
constexpr int kStW1Bytes = 3 * (kStK / 16) * 2 * 128 * 16;  // 98 304: W1 (128 x 128), N form
__host__ __device__ constexpr int st_w2_bytes(int c_out) { return 3 * (kStK / 16) * 2 * c_out * 16; }
constexpr int kStLdsBase = kStW1Bytes + 2 * 128 * 8;        // + (sc0, sh0) + (sc1, sh1)
// + (sc2, sh2) + the NS == 64 carry slots (4 waves x C_out / 32 blocks x 64 lanes)
__host__ __device__ constexpr int st_lds_bytes(int c_out) { return kStLdsBase + c_out * 8 + 4 * (c_out / 32) * 64 * 4; }

struct StoredArgs {
  int r;                 // columns per cloud (m * ns)
  int tiles_per_cloud;   // r / 32
  int total_tiles;       // b * r / 32
  int tpw;               // tiles per wave (1, or 2: NS == 64 always 2)
  const float *y0;       // (b, 128, r): layer 0's raw output
  const char *wimg;      // mlp_eval_stored_prepare's image: [W1 N form][W2 T form]
  const float *sc0, *sh0, *sc1, *sh1, *sc2, *sh2;
  float *out;            // (b, C_out, r / NS)
};

// W1 (128,128) -> N-form image (row = output channel, k slot (t, h, e) <-> input channel
// 16 t + 8 h + e); W2 (C_out,128) -> T-form image (k slot <-> input channel 16 t + 8 (e >> 2) +
// 4 h + (e & 3): the order layer 1's accumulators hold them in)
__global__ void __launch_bounds__(256)
eval_stored_prep_kernel(const float *__restrict__ w1, const float *__restrict__ w2, int c_out,
                        char *__restrict__ img) {
  constexpr int T = kStK / 16;
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g < 128 * T * 2) {
    const int row = g / (T * 2), th = g % (T * 2), t = th >> 1, hh = th & 1;
    const float *src = w1 + (size_t)row * kStK + 16 * t + 8 * hh;
    const Split3 s = split3(*reinterpret_cast<const float4 *>(src), *reinterpret_cast<const float4 *>(src + 4));
    store_frag(img + ((t * 2 + hh) * 128 + row) * 16, kStW1Bytes / 3, s);
  } else if (g < (128 + c_out) * T * 2) {
    const int q = g - 128 * T * 2;
    const int row = q / (T * 2), th = q % (T * 2), t = th >> 1, hh = th & 1;
    const float *src = w2 + (size_t)row * kStK + 16 * t + 4 * hh;
    const Split3 s = split3(*reinterpret_cast<const float4 *>(src), *reinterpret_cast<const float4 *>(src + 8));
    const int term = st_w2_bytes(c_out) / 3;
    store_frag(img + kStW1Bytes + ((t * 2 + hh) * c_out + row) * 16, term, s);
  }
}

template <int NS, int M2B>
__global__ void __launch_bounds__(256, 1) eval_stored_kernel(const StoredArgs a) {
  constexpr int M1 = 128, M2 = 32 * M2B, T = kStK / 16;
  constexpr int W1_TERM = kStW1Bytes / 3, W2_TERM = st_w2_bytes(M2) / 3;
  constexpr int HB = 4;                       // layer-2 blocks per half (128 channels)
  constexpr int HALVES = M2B / HB;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const char *w1img = lds;
  float2 *c0tab = reinterpret_cast<float2 *>(lds + kStW1Bytes);
  float2 *c1tab = reinterpret_cast<float2 *>(lds + kStW1Bytes + 128 * 8);
  float2 *c2tab = reinterpret_cast<float2 *>(lds + kStLdsBase);
  float *carry = reinterpret_cast<float *>(lds + kStLdsBase + M2 * 8);  // [wave][half][block][lane]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  {
    const uint4 *src = reinterpret_cast<const uint4 *>(a.wimg);
    uint4 *dst = reinterpret_cast<uint4 *>(lds);
    for (int i = tid; i < kStW1Bytes / 16; i += 256) dst[i] = src[i];
    if (tid < 128) {
      c0tab[tid] = make_float2(a.sc0[tid], a.sh0[tid]);
      c1tab[tid] = make_float2(a.sc1[tid], a.sh1[tid]);
    }
    for (int i = tid; i < M2; i += 256) c2tab[i] = make_float2(a.sc2[i], a.sh2[i]);
  }
  __syncthreads();

  const float2 *c0h = c0tab + 8 * h;
  const float2 *c1h = c1tab + 4 * h;
  const char *w1lane = w1img + (h * M1 + l31) * 16;
  const char *w2lane = a.wimg + kStW1Bytes + (h * M2 + l31) * 16;
  constexpr int TPG = NS > 32 ? NS / 32 : 1;

  const int tile0 = ((int)blockIdx.x * 4 + wave) * a.tpw;
#pragma unroll 1
  for (int it = 0; it < a.tpw; ++it) {
    const int tile = tile0 + it;
    if (tile >= a.total_tiles) break;  // (NS == 64: total and tile0 even, a group never splits)
    const int b = tile / a.tiles_per_cloud, col0 = (tile - b * a.tiles_per_cloud) * 32;

    // ---- this lane's 64 raw inputs of the tile: channel 16 t + 8 h + e, column col0 + l31
    float xr[T][8];
    {
      const float *p = a.y0 + ((size_t)b * kStK + 8 * h) * a.r + col0 + l31;
#pragma unroll
      for (int t = 0; t < T; ++t)
#pragma unroll
        for (int e = 0; e < 8; ++e) xr[t][e] = p[(size_t)(16 * t + e) * a.r];
    }
    // ---- layer 1 (N form): relu(bn0(y0)) at load
    f32x16 acc1[4];
    auto prep0 = [&](int t) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float2 c = c0h[16 * t + e];
        v[e] = fmaxf(__fmaf_rn(xr[t][e], c.x, c.y), 0.f);
      }
      return split3(v);
    };
    auto load_w1 = [&](int t, Split3 (&w)[4]) {
#pragma unroll
      for (int i = 0; i < 4; ++i) w[i] = lds_frag(w1lane + img_off<kStK, M1>(0, t, 0, 32 * i), W1_TERM);
    };
    {
      Split3 sc = prep0(0), wc[4];
      load_w1(0, wc);
#pragma unroll
      for (int t = 0; t < T; ++t) {
        Split3 sn = sc, wn[4] = {wc[0], wc[1], wc[2], wc[3]};
        if (t + 1 < T) {
          sn = prep0(t + 1);
          load_w1(t + 1, wn);
        }
        if (t == 0) mfma6<4, false, true>(acc1, sc, wc);
        else mfma6<4, false>(acc1, sc, wc);
        sc = sn;
#pragma unroll
        for (int i = 0; i < 4; ++i) wc[i] = wn[i];
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // ---- layer 2's operand: relu(bn1(acc1)) split once, kept for every half of C_out
    Split3 a2[T];
#pragma unroll
    for (int t = 0; t < T; ++t) a2[t] = ev_act_of_acc(acc1, t, c1h);

    // ---- layer 2 (T form), 128 output channels at a time (a loop, not unrolled: one half's
    // accumulators live at a time), W2 fragments from L2 one step ahead.  NS == 64: the first tile's
    // maxima wait in a wave-private LDS slot for the second tile of the group.
    const int p = it % TPG;
    const int groups = a.r / NS;
    const int g0 = NS == 16 ? col0 / 16 : (col0 - 32 * p) / NS;
#pragma unroll 1
    for (int hf = 0; hf < HALVES; ++hf) {
      f32x16 acc2[HB];
      const char *w2h = w2lane + hf * (HB * 32 * 16);
      auto load_w2 = [&](int t, Split3 (&w)[HB]) {
#pragma unroll
        for (int i = 0; i < HB; ++i) w[i] = lds_frag(w2h + img_off<kStK, M2>(0, t, 0, 32 * i), W2_TERM);
      };
      Split3 wc[HB];
      load_w2(0, wc);
#pragma unroll
      for (int t = 0; t < T; ++t) {
        Split3 wn[HB];
        if (t + 1 < T) load_w2(t + 1, wn);
        if (t == 0) mfma6<HB, true, true>(acc2, a2[t], wc);
        else mfma6<HB, true>(acc2, a2[t], wc);
        if (t + 1 < T) {
#pragma unroll
          for (int i = 0; i < HB; ++i) wc[i] = wn[i];
        }
        __builtin_amdgcn_sched_barrier(0);  // (no hoisting of later steps' loads: registers)
      }
      float best[HB][2];
      ev_pool<HB, NS>(acc2, c2tab, HB * hf, l31, best, 0);
      if constexpr (TPG == 2) {
        float *slot = carry + ((wave * HALVES + hf) * HB) * 64 + lane;
        if (p == 0) {
#pragma unroll
          for (int j = 0; j < HB; ++j) slot[64 * j] = best[j][0];
          continue;
        }
#pragma unroll
        for (int j = 0; j < HB; ++j) best[j][0] = fmaxf(best[j][0], slot[64 * j]);
      }
      ev_pool_store<HB, NS>(best, a.out, (size_t)b * M2 + 32 * HB * hf, groups, g0, l31, h);
    }
  }
}

bool stored_shape_ok(int b, int c_in, int c_mid, int c_out, int m, int ns) {
  if (b <= 0 || m <= 0 || c_in != 128 || c_mid != 128 || !(c_out == 128 || c_out == 256)) return false;
  if (!(ns == 16 || ns == 32 || ns == 64)) return false;
  const long long r = (long long)m * ns;
  return r % 32 == 0 && (long long)b * r * 128 < (1LL << 31) * 4LL && (long long)b * r < (1LL << 31);
}

// tiles per wave of the STORED launch: two where the chip is covered anyway (fewer LDS image loads;
// NS == 64 always, a group is two tiles), one otherwise
int stored_tiles_per_wave(int b, int m, int ns) {
  const long long total_tiles = (long long)b * m * ns / 32;
  return (ns == 64 || total_tiles >= 4 * 2 * 2 * pn2_cu_count()) ? 2 : 1;
}

template <typename Kern, typename Args>
void eval_launch(Kern kern, int wgs, size_t lds_bytes, hipStream_t stream, const Args &args) {
  // once per kernel (by address: the instantiations share one pointer type); the engine runs its
  // eager warm-up before it captures, so this happens outside any capture
  pn2_allow_dynamic_lds(reinterpret_cast<const void *>(kern), lds_bytes);
  hipLaunchKernelGGL(kern, dim3(wgs), dim3(256), lds_bytes, stream, args);
}

bool misaligned(const void *p) { return (reinterpret_cast<size_t>(p) & 15) != 0; }

}  // namespace

#define MLP_API extern "C" __attribute__((visibility("default")))

// 1 when mlp_eval_lin4_pool covers a 4 -> 64 -> 64 -> c_out module on a (b, 4, m, ns) grouped input
// (c_out 128, ns 16 / 32 / 64, m * ns a multiple of 256), else 0
MLP_API int mlp_eval_lin4_supported(int b, int c_in, int c_mid, int c_out, int m, int ns) {
  return (c_in == 4 && c_mid == 64 && c_out == 128 && lin4_shape_ok(b, m, ns)) ? 1 : 0;
}

// Eval-mode SA1 MLP + max-pool in one pass: x4 (b, 4, m * ns) grouped input, img the weight image
// mlp_chain_lin4_prepare made of (w0, sc0, sh0, w1, w2), (sc1, sh1) (64) and (sc2, sh2) (128) the
// folded BatchNorms of layers 1 and 2 -> out (b, 128, m).
MLP_API int mlp_eval_lin4_pool(int b, int m, int ns, const float *x4, const void *img, const float *sc1,
                               const float *sh1, const float *sc2, const float *sh2, float *out,
                               void *stream_) {
  if (!lin4_shape_ok(b, m, ns) || !x4 || !img || !sc1 || !sh1 || !sc2 || !sh2 || !out || misaligned(img))
    return (int)hipErrorInvalidValue;
  Lin4Args a = {};
  a.r = m * ns; a.tiles_per_cloud = a.r / 32;
  a.x4 = x4; a.wimg = (const char *)img;
  a.sc1 = sc1; a.sh1 = sh1; a.sc2 = sc2; a.sh2 = sh2; a.out = out;
  const int wgs = (int)((long long)b * (a.r / 32) / (4 * kL4TilesPerWave));
  hipStream_t stream = (hipStream_t)stream_;
  if (ns == 16) eval_launch(eval_lin4_kernel<16>, wgs, kL4Lds, stream, a);
  else if (ns == 32) eval_launch(eval_lin4_kernel<32>, wgs, kL4Lds, stream, a);
  else eval_launch(eval_lin4_kernel<64>, wgs, kL4Lds, stream, a);
  return pn2_launch_status();
}

// 1 when mlp_eval_stored_pool covers a c_in -> c_mid -> c_out tail (128 -> 128 -> 128 / 256) on a
// (b, 128, m, ns) raw layer-0 output (ns 16 / 32 / 64, m * ns a multiple of 32), else 0
MLP_API int mlp_eval_stored_supported(int b, int c_in, int c_mid, int c_out, int m, int ns) {
  return stored_shape_ok(b, c_in, c_mid, c_out, m, ns) ? 1 : 0;
}

// tiles per wave (1 or 2) of mlp_eval_stored_pool's launch on this shape, 0 where it is unsupported
MLP_API int mlp_eval_stored_tiles_per_wave(int b, int c_out, int m, int ns) {
  return stored_shape_ok(b, 128, 128, c_out, m, ns) ? stored_tiles_per_wave(b, m, ns) : 0;
}

// bytes of the weight image mlp_eval_stored_prepare fills (c_out 128 / 256)
MLP_API size_t mlp_eval_stored_image_bytes(int c_out) {
  return (c_out == 128 || c_out == 256) ? (size_t)(kStW1Bytes + st_w2_bytes(c_out)) : 0;
}

// w1 (128,128), w2 (c_out,128) -> img: fragment-ordered bf16 images (exact three-term split)
MLP_API int mlp_eval_stored_prepare(int c_out, const float *w1, const float *w2, void *img, void *stream_) {
  if (!(c_out == 128 || c_out == 256) || !w1 || !w2 || !img || misaligned(w1) || misaligned(w2) ||
      misaligned(img))
    return (int)hipErrorInvalidValue;
  const int items = (128 + c_out) * (kStK / 16) * 2;
  hipLaunchKernelGGL(eval_stored_prep_kernel, dim3((items + 255) / 256), dim3(256), 0, (hipStream_t)stream_,
                     w1, w2, c_out, (char *)img);
  return pn2_launch_status();
}

// Eval-mode tail of a pooled MLP in one pass: y0 (b, 128, m * ns) raw layer-0 output, (sc0, sh0) its
// folded BatchNorm, img = mlp_eval_stored_prepare, (sc1, sh1) / (sc2, sh2) folded BatchNorms of
// layers 1 / 2 -> out (b, c_out, m).
MLP_API int mlp_eval_stored_pool(int b, int c_out, int m, int ns, const float *y0, const float *sc0,
                                 const float *sh0, const void *img, const float *sc1, const float *sh1,
                                 const float *sc2, const float *sh2, float *out, void *stream_) {
  if (!stored_shape_ok(b, 128, 128, c_out, m, ns) || !y0 || !sc0 || !sh0 || !img || !sc1 || !sh1 || !sc2 ||
      !sh2 || !out || misaligned(img))
    return (int)hipErrorInvalidValue;
  StoredArgs a = {};
  a.r = m * ns; a.tiles_per_cloud = a.r / 32;
  a.total_tiles = (int)((long long)b * a.tiles_per_cloud);
  a.tpw = stored_tiles_per_wave(b, m, ns);
  a.y0 = y0; a.wimg = (const char *)img;
  a.sc0 = sc0; a.sh0 = sh0; a.sc1 = sc1; a.sh1 = sh1; a.sc2 = sc2; a.sh2 = sh2; a.out = out;
  const int wgs = pn2_ceil_div(a.total_tiles, 4 * a.tpw);
  const size_t lds = (size_t)st_lds_bytes(c_out);
  hipStream_t stream = (hipStream_t)stream_;
#define EV_ST(NS_, B_) eval_launch(eval_stored_kernel<NS_, B_>, wgs, lds, stream, a)
  if (c_out == 256) {
    if (ns == 16) EV_ST(16, 8); else if (ns == 32) EV_ST(32, 8); else EV_ST(64, 8);
  } else {
    if (ns == 16) EV_ST(16, 4); else if (ns == 32) EV_ST(32, 4); else EV_ST(64, 4);
  }
#undef EV_ST
  return pn2_launch_status();
}
