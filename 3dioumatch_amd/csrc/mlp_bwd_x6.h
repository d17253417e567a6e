// 3dioumatch_amd/csrc/mlp_bwd_x6.h (included by mlp_bwd_fused.hip) -- the one-pass backward of a shared-MLP layer (see
// mlp_bwd_fused.hip for what it computes: dQ = W^T P and dW = sum P Q^T from ONE staging of the
// chunk) with its fp32 products on the bf16 matrix pipe (mlp_frag.h: exact three-term split,
// six of the nine partial products, v_mfma_f32_32x32x16_bf16).
//
// The fp32 kernel gathers a fragment as single floats from odd-pitch fp32 tiles; splitting those
// fragments in registers costs more vector-ALU time than the matrix pipe saves (every wave
// splits the same P fragments again).  Here every element is split ONCE, when it is staged:
//   * LDS holds, per term (hi / mid / lo), a row-major bf16 image of the chunk: P[m][n] and
//     Q[k][n], n contiguous, row pitch 80 bytes for 32 columns (80 / 16 odd: the 16-byte
//     row-wise reads of 16 consecutive rows fall on 16 distinct bank groups).  A staging lane
//     owns 16 consecutive n of one row: two 16-byte stores per term.
//   * wgrad (reduction over n): the A operand of lane (row m, eight consecutive n) and the B
//     operand (row k of Q, the same n) are ONE ds_read_b128 per term each.
//   * dgrad (reduction over m) needs, for column n, eight consecutive m -- the transpose of the
//     image.  ds_read_b64_tr_b16 does it in the LDS crossbar: the 16 lanes of a group hand in
//     the addresses of a 4 (m) x 16 (n) block as sixteen 8-byte pieces, lane i the piece
//     (m = i >> 2, n = 4 (i & 3) ..), and lane l receives column l & 15 of the block, its four m
//     (measured on the part, tools/micro: out[l][j] = piece[(l >> 2) + 4 j][l & 3]); two reads
//     per term give the lane's eight m.  No second copy of P.
//   * W^T (the A operand of dgrad) is split once per kernel and lives in registers.
// One workgroup per CU (the images are double buffered: 120 KB at M = K = 128), persistent over
// a contiguous range of 32-column chunks; staging of chunk c+1 and the loads of chunk c+2 are
// slotted between the MFMA groups of chunk c as in the fp32 kernel.
//
// The workgroup has EIGHT waves, two per SIMD, with fixed roles: waves 0-3 compute dQ (and the sums of
// the layer below), waves 4-7 dW; the staging is shared out between the roles by a compile-time
// table.  All eight share one set of images and meet at one barrier per chunk.  Workgroup count,
// chunk ranges, image layout and the order in which every accumulator receives its terms are those
// of the earlier four-wave form (every wave did dgrad, then wgrad, and an eighth of the staging):
// the results are bit-identical to it (profiles/x6_roles_bit_identity.json).  Measured
// (profiles/x6_roles_kernel.json, x6_roles_step_ab.json): all four instantiations are faster in
// this form, none keeps the old body -- 189 -> 172 us at SA2's layer 2, 197 -> 166 at the IoU
// branch's pooled layer, 48 -> 36 at the vote aggregation; 624 -> 522 us per train step over the
// kernel's seven launches.  No instantiation touches scratch memory any more (the four-wave forms
// with the sums spilled 10 and 23 registers inside the chunk loop).  What the kernel still waits for
// is its loads: 128-byte row pieces at 3.3 TB/s; loads two chunks ahead (a second register set),
// s_setprio 1 for waves 4-7 and other staging tables were measured and gained nothing.
#pragma once
#include "common.h"
#include "mlp_operand.h"
#include <type_traits>

namespace {

#if defined(BWDX6_ABL) && BWDX6_ABL == 2   // (timing ablation 2: no MFMAs)
#define mfma_x6(ACC, A, B) do { (ACC)[0] += __builtin_bit_cast(float, (int)(A).hi[0] + (int)(B).hi[0] + (int)(A).mid[1] + (int)(B).mid[1] + (int)(A).lo[2] + (int)(B).lo[2]); } while (0)
#endif

// Which waves stage which slices (a slice = 32 rows of P or Q, one float4 per lane of a role's 256):
// bit sl set = the dgrad waves stage slice sl (P slices 0 .. PS-1, then the Q slices), clear = the
// wgrad waves do.  The wgrad waves have the loose register budget and no sums, so they take the P
// slices (two loads and the BatchNorm-backward transform each); the dgrad waves take two Q slices
// beside the sums, all four without them.  With the sums the tables 0xC0, 0xF0 and 0x03 measure
// within 2-3 % of each other at SA2's shape, "the wgrad waves stage everything" (0x00) 3 % slower,
// 0x0F spills (profiles/x6_roles_kernel.json); the table of the forms without the sums follows the
// instruction counts and was not varied (no layer of the train step runs them).
#ifndef BWDX6_DGRAD_SLICES_STATS
#define BWDX6_DGRAD_SLICES_STATS 0xC0u
#endif
#ifndef BWDX6_DGRAD_SLICES_PLAIN
#define BWDX6_DGRAD_SLICES_PLAIN 0xF0u
#endif

constexpr int x6_popcount(unsigned v) { return v == 0 ? 0 : (int)(v & 1u) + x6_popcount(v >> 1); }

// MB = M / 32 (4 or 8: a wave owns MB / 4 row blocks of dW), KB = 32-column blocks of dW / rows
// blocks of Q (K padded), KBD = 32-row blocks of dQ through the matrix cores (rows xyz ..)
// STATS: also the BatchNorm-backward sums of the layer BELOW (the one whose relu(bn(.)) output is Q),
// s1 = sum g, s2 = sum g * xhat with g = dQ * [y*sc + sh > 0], xhat = (y - mu) * is, from the dQ
// blocks in the accumulators and a raw fp32 copy of the Q rows kept next to the images (the same
// arithmetic as the separate pass bn_relu_bwd_partial over (y, dQ), which it replaces):
// stats_part (k, workgroups, 2).
//
// One role of the workgroup (DGRAD: waves 0-3, else waves 4-7; `wave` = 0..3 within the role, `tid`
// = 0..255 within the role).  Setup, chunk loop and epilogue are written per role, so that a role
// keeps only its own long-lived registers (dgrad: W^T fragments + sums; wgrad: the dW blocks).
template <int MB, int KB, int KBD, int PMODE, int QMODE, bool STATS, bool DGRAD>
__device__ __forceinline__ void gemm_bwd_x6_role(int k_total, int r, int total_chunks,
                                                 int chunks_per_cloud, int xyz, const OperandB &P,
                                                 const OperandB &Q, const float *__restrict__ w,
                                                 float *__restrict__ dq, float *__restrict__ part,
                                                 float *__restrict__ stats_part, char *lds, int tid,
                                                 int wave) {
  constexpr int M = 32 * MB, KP = 32 * KB, TN = 32;
  constexpr int RP = TN * 2 + 16;              // row pitch of an image in bytes
  constexpr int PIMG = M * RP, QIMG = KP * RP;  // bytes per term
  constexpr int RAWP = (TN + 4) * 4;           // row pitch of the raw Q copy (STATS), bytes
  constexpr int QRAW = STATS ? KP * RAWP : 0;
  constexpr int BUF = 3 * (PIMG + QIMG) + QRAW;
  constexpr int RCOFF = 2 * BUF;               // float4 (sc, sh, mu, is) per Q row (STATS)
  static_assert(2 * BUF + (STATS ? KP * 16 : 0) <= 160 * 1024, "two buffers of images must fit the LDS");
  static_assert(!STATS || QMODE == OP_BNRELU, "the sums are those of a BatchNorm+ReLU layer below");
  static_assert(MB % 4 == 0 && KBD % 4 == 0, "blocks split over four waves");
  constexpr int WMB = MB / 4, WKB = KB;        // dW blocks per wave: rows wave + 4 i, all columns
  constexpr int DK = KBD / 4;                  // dQ row blocks per wave (one column block: TN = 32)
  constexpr int DG = M / 16, WG = TN / 16;     // MFMA steps of dgrad / wgrad per chunk
  // staging: a slice is one float4 (four columns) per lane; the 8 lanes of a row cover its 128
  // bytes, so that a load instruction touches whole cache lines (32 rows per slice of 256 lanes)
  constexpr int PS = M / 32, QS = KP / 32;     // slices of P / Q per chunk
  constexpr int NS = PS + QS;
  constexpr unsigned DMASK = (STATS ? BWDX6_DGRAD_SLICES_STATS : BWDX6_DGRAD_SLICES_PLAIN) & ((1u << NS) - 1u);
  constexpr unsigned MINE = DGRAD ? DMASK : (~DMASK & ((1u << NS) - 1u));  // this role's slices
  constexpr int NOWN = x6_popcount(MINE);
  constexpr int NG = DGRAD ? DG : WG * WKB;    // this role's slots between MFMA groups
#define X6_MINE(sl) (((MINE >> (sl)) & 1u) != 0u)

  const int lane = tid & 63;
  const int l31 = lane & 31, lhi = lane >> 5;
  const int seg_row = tid >> 3, seg_c = (tid & 7) * 4;  // row within a slice, first column

  RowCoef pc[PS], qc[QS];
  bool q_ok[QS];
  size_t p_lane[PS], q_lane[QS];
#pragma unroll
  for (int p = 0; p < PS; ++p) {
    if (!X6_MINE(p)) continue;
    pc[p] = load_row_coef<PMODE>(P, seg_row + p * 32, true);
    p_lane[p] = (size_t)(seg_row + p * 32) * r + seg_c;
  }
#pragma unroll
  for (int q = 0; q < QS; ++q) {
    if (!X6_MINE(PS + q)) continue;
    const int row = seg_row + q * 32;
    q_ok[q] = row < k_total;
    qc[q] = load_row_coef<QMODE>(Q, q_ok[q] ? row : k_total - 1, true);
    q_lane[q] = (size_t)(q_ok[q] ? row : k_total - 1) * r + seg_c;
  }
  // pooled form: the lane's four columns lie in group (col0 / ns) + lane_g, from sample
  // (col0 % ns) + lane_s on (ns a multiple of 4 that divides 32 or is divided by it)
  const int lane_g = PMODE == OP_POOLDY ? seg_c / P.ns : 0;
  const int lane_s = PMODE == OP_POOLDY ? seg_c % P.ns : 0;

  // dgrad role, per lane: column l31 of the 16 accumulator rows of every dQ block, over all chunks
  float st1[DK][STATS && DGRAD ? 16 : 1], st2[DK][STATS && DGRAD ? 16 : 1];
#pragma unroll
  for (int e = 0; e < DK; ++e)
#pragma unroll
    for (int q = 0; q < (STATS && DGRAD ? 16 : 1); ++q) { st1[e][q] = 0.f; st2[e][q] = 0.f; }

  // dgrad role: W^T fragments of this wave's dQ row blocks, split once: step s holds
  // m = 16 s + 8 lhi + (0..7)
  Split3 wsp[DK][DG];
  if (DGRAD) {
#pragma unroll
    for (int e = 0; e < DK; ++e) {
      const float *wc = w + xyz + 32 * (wave * DK + e) + l31;
#pragma unroll
      for (int s = 0; s < DG; ++s) {
        float w8[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) w8[j] = wc[(size_t)(16 * s + 8 * lhi + j) * k_total];
        wsp[e][s] = split3(w8);
      }
    }
  }

  // wgrad role: the dW blocks of this wave
  f32x16 accW[WMB][WKB];
  if (!DGRAD) {
#pragma unroll
    for (int i = 0; i < WMB; ++i)
#pragma unroll
      for (int j = 0; j < WKB; ++j)
#pragma unroll
        for (int q = 0; q < 16; ++q) accW[i][j][q] = 0.f;
  }

  const int per = (total_chunks + (int)gridDim.x - 1) / (int)gridDim.x;
  const int c_lo = (int)blockIdx.x * per;
  const int c_hi = c_lo + per < total_chunks ? c_lo + per : total_chunks;

  // raw operands of this role's slices of one chunk in registers: a slice of chunk c+1 is staged
  // from them between two MFMA groups of chunk c and reloaded with chunk c+2 right away.
  float4 px[PS], pd[PS], qx[QS];
  int pwin[PS];
  float pdp[PS];
#pragma unroll
  for (int p = 0; p < PS; ++p) {
    pwin[p] = -1; pdp[p] = 0.f;
    px[p] = make_float4(0.f, 0.f, 0.f, 0.f); pd[p] = px[p];
  }
#pragma unroll
  for (int q = 0; q < QS; ++q) qx[q] = make_float4(0.f, 0.f, 0.f, 0.f);

  struct ChunkAt { size_t p, q, grp; int s0; };
  auto chunk_at = [&](int c) {
    const int b = c / chunks_per_cloud;
    const int col0 = (c - b * chunks_per_cloud) * TN;
    ChunkAt at;
    at.p = (size_t)b * M * r + col0;
    at.q = (size_t)b * k_total * r + col0;
    at.grp = 0; at.s0 = 0;
    if (PMODE == OP_POOLDY) {
      const int g0 = col0 / P.ns;
      at.grp = (size_t)b * M * P.groups + g0;
      at.s0 = col0 - g0 * P.ns;
    }
    return at;
  };
  auto fetch_slice = [&](int sl, const ChunkAt &at) {
    if (sl < PS) {
      const int p = sl;
      px[p] = *reinterpret_cast<const float4 *>(P.x + at.p + p_lane[p]);
      if (PMODE == OP_DY) {
        pd[p] = *reinterpret_cast<const float4 *>(P.dz + at.p + p_lane[p]);
      } else if (PMODE == OP_POOLDY) {
        const size_t gi = at.grp + (size_t)(seg_row + p * 32) * P.groups + lane_g;
        pwin[p] = P.argmax[gi] - (at.s0 + lane_s);
        pdp[p] = P.dz[gi];
      }
    } else {
      const int q = sl - PS;
      qx[q] = *reinterpret_cast<const float4 *>(Q.x + at.q + q_lane[q]);
    }
  };
  // slice: four consecutive n of a row -> transformed, split, 8 bytes per term into the images
  auto stage_slice = [&](int sl, int buf) {
    char *base = lds + (size_t)buf * BUF;
    if (sl < PS) {
      const int p = sl;
      const float xv[4] = {px[p].x, px[p].y, px[p].z, px[p].w};
      const float dv[4] = {pd[p].x, pd[p].y, pd[p].z, pd[p].w};
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float dz = PMODE == OP_POOLDY ? (e == pwin[p] ? pdp[p] : 0.f) : dv[e];
        v[e] = transform<PMODE>(xv[e], dz, pc[p]);
      }
      store_split4<RP>(base, PIMG, seg_row + p * 32, seg_c, v);
    } else {
      const int q = sl - PS;
      const float xv[4] = {qx[q].x, qx[q].y, qx[q].z, qx[q].w};
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = q_ok[q] ? transform<QMODE>(xv[e], 0.f, qc[q]) : 0.f;
      store_split4<RP>(base + 3 * PIMG, QIMG, seg_row + q * 32, seg_c, v);
      if (STATS)
        *reinterpret_cast<float4 *>(base + 3 * (PIMG + QIMG) + (size_t)(seg_row + q * 32) * RAWP + seg_c * 4) =
            qx[q];
    }
  };

  auto clampc = [&](int c) { return c < c_hi ? c : c_hi - 1; };  // (surplus loads are never consumed)
  if (NOWN > 0 && c_lo < c_hi) {
    const ChunkAt first = chunk_at(c_lo), second = chunk_at(clampc(c_lo + 1));
#pragma unroll
    for (int sl = 0; sl < NS; ++sl)
      if (X6_MINE(sl)) fetch_slice(sl, first);
#pragma unroll
    for (int sl = 0; sl < NS; ++sl) {
      if (!X6_MINE(sl)) continue;
      stage_slice(sl, 0);
      fetch_slice(sl, second);
    }
  }
  __syncthreads();

  // lane constants of the fragment reads
  // dgrad B (transposing): piece of lane i in its group of 16: m = 4 r + (i >> 2), n = 16 gn + 4 (i & 3)
  const int tr_off = (8 * lhi + ((lane & 15) >> 2)) * RP + (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;
  // wgrad A / B (row-wise): row = block * 32 + l31, n = 16 s + 8 lhi
  const int rw_off = l31 * RP + 8 * lhi * 2;

  // one chunk of this role: MFMAs on buffer `cur`, its slices of chunk c+1 into the other buffer
  auto chunk = [&](int c, int cur) {
    const char *Pc = lds + (size_t)cur * BUF, *Qc = Pc + 3 * PIMG;
    const ChunkAt ahead = chunk_at(clampc(c + 2));
    // slot g of NG: the role's owned slices in order, spread evenly over its MFMA groups
    auto between = [&](int g) {
#if !defined(BWDX6_ABL) || BWDX6_ABL != 1   // (timing ablation 1: no staging / loads in the loop)
      int own = 0;
#pragma unroll
      for (int sl = 0; sl < NS; ++sl) {
        if (!X6_MINE(sl)) continue;
        if (own >= g * NOWN / NG && own < (g + 1) * NOWN / NG) {
#if !defined(BWDX6_ABL) || BWDX6_ABL != 7
          stage_slice(sl, cur ^ 1);
#else   // (timing ablation 7: loads without staging -- the loaded registers are waited for, no more)
          if (sl < PS) asm volatile("" :: "v"(px[sl].x), "v"(px[sl].w), "v"(pd[sl].x), "v"(pd[sl].w), "v"(pdp[sl]), "v"(pwin[sl]));
          else asm volatile("" :: "v"(qx[sl - PS].x), "v"(qx[sl - PS].w));
#endif
#if !defined(BWDX6_ABL) || BWDX6_ABL != 6   // (timing ablation 6: staging, no loads)
          fetch_slice(sl, ahead);
#endif
        }
        ++own;
      }
#endif
    };

    if (DGRAD) {
      const int b = c / chunks_per_cloud;
      const int col0 = (c - b * chunks_per_cloud) * TN;
      // ---- dQ block (rows k) = W^T (registers) * P (transposing reads), fragments one step
      // ahead of the MFMAs
      f32x16 accD[DK];
#pragma unroll
      for (int e = 0; e < DK; ++e)
#pragma unroll
        for (int q = 0; q < 16; ++q) accD[e][q] = 0.f;
      bf16x4 pf[2][3][2];  // [ring][term][half of the eight m]
      auto frag = [&](int s, bf16x4 (&dst)[3][2]) {
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          const char *p0 = Pc + (size_t)t * PIMG + (size_t)(16 * s) * RP + tr_off;
          dst[t][0] = lds_read_tr(p0);
          dst[t][1] = lds_read_tr(p0 + 4 * RP);
        }
      };
#if defined(BWDX6_ABL) && BWDX6_ABL == 3   // (timing ablation 3: no dgrad)
#pragma unroll
      for (int s = 0; s < DG; ++s) between(s);
#else
      frag(0, pf[0]);
#pragma unroll
      for (int s = 0; s < DG; ++s) {
        if (s + 1 < DG) frag(s + 1, pf[(s + 1) & 1]);
        Split3 sb;
        sb.hi = __builtin_shufflevector(pf[s & 1][0][0], pf[s & 1][0][1], 0, 1, 2, 3, 4, 5, 6, 7);
        sb.mid = __builtin_shufflevector(pf[s & 1][1][0], pf[s & 1][1][1], 0, 1, 2, 3, 4, 5, 6, 7);
        sb.lo = __builtin_shufflevector(pf[s & 1][2][0], pf[s & 1][2][1], 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
        for (int e = 0; e < DK; ++e) mfma_x6(accD[e], wsp[e][s], sb);
        between(s);
      }
#endif
#if !defined(BWDX6_ABL) || (BWDX6_ABL != 5 && BWDX6_ABL != 3)   // (timing ablation 5: no dQ stores)
#pragma unroll
      for (int e = 0; e < DK; ++e) {
        const int kbd = wave * DK + e;
        float *dst = dq + ((size_t)b * k_total + xyz + 32 * kbd + 4 * lhi) * r + col0 + l31;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
#if defined(BWDX6_PLAIN_STORES)
          dst[(size_t)((q & 3) + 8 * (q >> 2)) * r] = accD[e][q];
#else
          __builtin_nontemporal_store(accD[e][q], &dst[(size_t)((q & 3) + 8 * (q >> 2)) * r]);
#endif
        }
      }
#endif
      if (STATS) {
        // every accumulator row of the dQ blocks: this lane holds column l31 and rows
        // 32*kbd + 4*lhi + (q&3) + 8*(q>>2)
        const float4 *rc = reinterpret_cast<const float4 *>(lds + RCOFF);
        const char *raw = Pc + 3 * (PIMG + QIMG);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int ro = (q & 3) + 8 * (q >> 2);
#pragma unroll
          for (int e = 0; e < DK; ++e) {
            const int row = 32 * (wave * DK + e) + 4 * lhi + ro;
            const float4 c4 = rc[row];
            const float yv = *reinterpret_cast<const float *>(raw + (size_t)row * RAWP + l31 * 4);
            const float g = __fmaf_rn(yv, c4.x, c4.y) > 0.f ? accD[e][q] : 0.f;
            st1[e][q] += g;
            st2[e][q] = __fmaf_rn(g, (yv - c4.z) * c4.w, st2[e][q]);
          }
        }
      }
    } else {
      // ---- dW blocks += P * Q^T (row-wise reads of both images): P rows of this wave (per step),
      // Q column blocks one ahead
      Split3 sp[WMB], sq[2];
      auto pfrag = [&](int s) {
#pragma unroll
        for (int i = 0; i < WMB; ++i) {
          const char *p0 = Pc + (size_t)((wave + 4 * i) * 32) * RP + rw_off + 16 * s * 2;
          sp[i].hi = *reinterpret_cast<const bf16x8 *>(p0);
          sp[i].mid = *reinterpret_cast<const bf16x8 *>(p0 + PIMG);
          sp[i].lo = *reinterpret_cast<const bf16x8 *>(p0 + 2 * PIMG);
        }
      };
      auto qfrag = [&](int u, Split3 &dst) {  // u = s * WKB + j
        const int s = u / WKB, j = u % WKB;
        const char *q0 = Qc + (size_t)(j * 32) * RP + rw_off + 16 * s * 2;
        dst.hi = *reinterpret_cast<const bf16x8 *>(q0);
        dst.mid = *reinterpret_cast<const bf16x8 *>(q0 + QIMG);
        dst.lo = *reinterpret_cast<const bf16x8 *>(q0 + 2 * QIMG);
      };
#if defined(BWDX6_ABL) && BWDX6_ABL == 4   // (timing ablation 4: no wgrad)
#pragma unroll
      for (int u = 0; u < WG * WKB; ++u) between(u);
#else
      pfrag(0);
      qfrag(0, sq[0]);
#pragma unroll
      for (int u = 0; u < WG * WKB; ++u) {
        const int s = u / WKB, j = u % WKB;
        if (u + 1 < WG * WKB) qfrag(u + 1, sq[(u + 1) & 1]);
#pragma unroll
        for (int i = 0; i < WMB; ++i) mfma_x6(accW[i][j], sp[i], sq[u & 1]);
        if (j == WKB - 1 && s + 1 < WG) pfrag(s + 1);  // (the MFMAs above hold their operands already)
        between(u);
      }
#endif
    }
    __syncthreads();  // chunk c read by all eight waves, chunk c+1 staged by its owners
  };
  for (int c = c_lo; c < c_hi; c += 2) {
    chunk(c, 0);
    if (c + 1 < c_hi) chunk(c + 1, 1);
  }

  if (DGRAD) {
    if (STATS && stats_part != nullptr) {
      // the lanes' column sums -> row sums through LDS (the image buffers are free: the chunk loop's
      // last barrier is behind every wave, and each wave parks and reads only its own rows)
      const int parts = (int)gridDim.x;
      float2 *park = reinterpret_cast<float2 *>(lds) + (size_t)wave * (32 * DK) * 33;
#pragma unroll
      for (int e = 0; e < DK; ++e)
#pragma unroll
        for (int q = 0; q < (STATS ? 16 : 1); ++q) {
          const int lrow = 32 * e + 4 * lhi + (q & 3) + 8 * (q >> 2);
          park[lrow * 33 + l31] = make_float2(st1[e][q], st2[e][q]);
        }
      for (int t = lane; t < 32 * DK; t += kWave) {  // (same wave wrote: LDS operations complete in order)
        float a1 = 0.f, a2 = 0.f;
        for (int c2 = 0; c2 < 32; ++c2) { const float2 v = park[t * 33 + c2]; a1 += v.x; a2 += v.y; }
        const int row = 32 * wave * DK + t;
        stats_part[((size_t)row * parts + blockIdx.x) * 2] = a1;
        stats_part[((size_t)row * parts + blockIdx.x) * 2 + 1] = a2;
      }
    }
  } else {
    float *out = part + (size_t)blockIdx.x * M * k_total;
#pragma unroll
    for (int i = 0; i < WMB; ++i) {
      const int mb = wave + 4 * i;
#pragma unroll
      for (int j = 0; j < WKB; ++j) {
        const int colk = j * 32 + l31;
        if (colk >= k_total) continue;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int row = mb * 32 + (q & 3) + 8 * (q >> 2) + 4 * lhi;
          out[(size_t)row * k_total + colk] = accW[i][j][q];
        }
      }
    }
  }
#undef X6_MINE
}

// 512 threads, two waves per SIMD with fixed roles: waves 0-3 the data gradient (and the sums), waves
// 4-7 the weight gradient.  Waves w and w + 4 share a SIMD, so every SIMD runs one wave of each role:
// the vector work of one (staging, dQ stores, sums) issues beside the MFMAs of the other.  Both
// roles share ONE set of images and meet at one barrier per chunk.
template <int MB, int KB, int KBD, int PMODE, int QMODE, bool STATS>
__global__ void __launch_bounds__(512, 1)
gemm_bwd_x6_kernel(int k_total, int r, int total_chunks, int chunks_per_cloud, int xyz,
                   OperandB opp, OperandB opq, const float *__restrict__ w,
                   float *__restrict__ dq, float *__restrict__ part,
                   float *__restrict__ stats_part) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  if (STATS) {
    constexpr int KP = 32 * KB;
    constexpr int RCOFF = 2 * (3 * (32 * MB + KP) * 80 + KP * 144);
    float4 *rc = reinterpret_cast<float4 *>(lds + RCOFF);
    for (int t = threadIdx.x; t < KP; t += 512)
      rc[t] = t < k_total ? make_float4(opq.scale[t], opq.shift[t], opq.mean[t], opq.invstd[t])
                          : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (wave < 4) {
    gemm_bwd_x6_role<MB, KB, KBD, PMODE, QMODE, STATS, true>(
        k_total, r, total_chunks, chunks_per_cloud, xyz, opp, opq, w, dq, part, stats_part, lds,
        (int)threadIdx.x, wave);
  } else {
    gemm_bwd_x6_role<MB, KB, KBD, PMODE, QMODE, STATS, false>(
        k_total, r, total_chunks, chunks_per_cloud, xyz, opp, opq, w, dq, part, stats_part, lds,
        (int)threadIdx.x - 256, wave - 4);
  }
}

}  // namespace

// workgroups of the bf16-split backward for a (128,128) layer of b clouds x r columns (one per CU,
// at least 8 chunks each), or 0 when that kernel does not run (not this shape)
static int mlp_bwd_x6_workgroups(int b, int m, int k, int r, int cus) {
  if (!(m == 128 && k == 128) || r % 32 != 0 || b <= 0) return 0;
  const long long total = (long long)b * (r / 32);
  long long g = cus;
  if (g > total / 8) g = total / 8;
  return (int)(g < 1 ? 1 : g);
}

// Launch the bf16-split backward for the shapes it covers (xyz == 0 forms); returns -1 when the
// shape is not covered (the caller then runs the fp32 kernel), else the launch status.
// stats_part (k, workgroups, 2) or null: the BatchNorm-backward sums of the layer below.
static int mlp_bwd_x6_try(int b, int m, int k, int r, int pmode, int qmode, const OperandB &P,
                          const OperandB &Q, const float *w, float *dq, float *part,
                          float *stats_part, int cus, int *workgroups, hipStream_t stream) {
  const int g = mlp_bwd_x6_workgroups(b, m, k, r, cus);
  if (g == 0 || qmode != OP_BNRELU || dq == nullptr) return -1;
  const int total_chunks = b * (r / 32), chunks_per_cloud = r / 32;
  *workgroups = g;
  constexpr int RP = 80;
#define BWDX6(MB, KB, KBD, PM, QM, ST)                                                              \
  do {                                                                                              \
    const size_t lds_bytes = 2 * (3 * (size_t)(m + k) * RP + (ST ? (size_t)k * 144 : 0)) +         \
                             (ST ? (size_t)k * 16 : 0);                                             \
    auto kern = gemm_bwd_x6_kernel<MB, KB, KBD, PM, QM, ST>;                                        \
    pn2_allow_dynamic_lds(reinterpret_cast<const void *>(kern), lds_bytes);                         \
    hipLaunchKernelGGL(kern, dim3(g), dim3(512), lds_bytes, stream, k, r, total_chunks,             \
                       chunks_per_cloud, 0, P, Q, w, dq, part, stats_part);                         \
  } while (0)
  const bool st = stats_part != nullptr;
  if (pmode == OP_DY && st) BWDX6(4, 4, 4, OP_DY, OP_BNRELU, true);
  else if (pmode == OP_DY) BWDX6(4, 4, 4, OP_DY, OP_BNRELU, false);
  else if (pmode == OP_POOLDY && st) BWDX6(4, 4, 4, OP_POOLDY, OP_BNRELU, true);
  else if (pmode == OP_POOLDY) BWDX6(4, 4, 4, OP_POOLDY, OP_BNRELU, false);
  else return -1;
#undef BWDX6
  return pn2_launch_status();
}
