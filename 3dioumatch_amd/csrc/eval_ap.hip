// 3dioumatch_amd/csrc/eval_ap.hip -- the AP evaluation without a host round trip per batch (gfx950).
//
// eval_match: eval_det_cls' per-detection loop (utils/eval_det.py:128-141) for one batch in its
// dense layout.  The host path flattens Python lists into (detection, ground-truth range) records
// and computes box3d_iou once per (proposal, class) detection; with per_class_proposal the 18 / 10
// detections of a proposal share one box, so here a workgroup owns a scene and a tile of
// kMatchRows proposals, a lane per (proposal, ground-truth slot) pair writes the pair's IoU into an
// LDS tile of 64 ground-truth columns ONCE, and after a barrier a lane per (proposal, class) slot
// scans the tile in ascending g under the strict `>` update, looking only at the columns of its
// class.  G > 64 loops over tiles and carries (best, arg) in the slot's lane.  The class filter
// compares against a per-column class in LDS; nothing is indexed by a runtime class in registers.
// The IoU itself is eval_box_iou.h, the code corners_best_match_kernel runs.
//
// eval_mark: eval_det.py:119-157 and voc_ap (:29-61) for every (class, threshold) in one launch,
// one workgroup each, over detections the caller has ordered by (class, score descending,
// insertion).  The greedy "first detection to claim a ground-truth box" is an integer minimum of
// the rank per ground-truth id (atomicMin: independent of the order the lanes arrive in), the
// cumulative sums are integer wave ballots, and rec / prec / the envelope are the host path's
// float64 expressions.
#include "eval_box_iou.h"
#include "../../include/iou3d_hip.h"
#include <float.h>
#include <limits.h>

namespace {

constexpr int kMatchRows = 4;    // proposals per workgroup
constexpr int kMatchCols = 64;   // ground-truth columns per LDS tile (MAX_NUM_OBJ of both datasets)
constexpr int kMatchThreads = kMatchRows * kMatchCols;
static_assert(kMatchRows * IOU3D_EVAL_MAX_CLASS <= kMatchThreads, "one slot per lane");

__global__ __launch_bounds__(kMatchThreads)
void eval_match_kernel(const EvalMatchArgs a) {
  __shared__ double tile[kMatchRows][kMatchCols];
  __shared__ int col_cls[kMatchCols];  // class of the column's box, -1: no valid box there
  const int t = threadIdx.x, b = blockIdx.y, k0 = blockIdx.x * kMatchRows;
  const int K = a.K, G = a.G, cm = a.C > 0 ? a.C : 1;

  // phase-1 role: the pair (row pk, column pg)
  const int pr = t / kMatchCols, pg = t % kMatchCols, pk = k0 + pr;
  const bool p_kept = pk < K && a.keep[(long long)b * K + pk] != 0;
  float cd[24];
  if (p_kept) load_box(a.det + ((long long)b * K + pk) * 24, cd);

  // phase-2 role: the slot (row sr, class sc)
  const int sr = t / cm, sc = t % cm, sk = k0 + sr;
  const bool s_live = sr < kMatchRows && sk < K;
  int want = -2;  // never a column's class
  if (s_live && a.keep[(long long)b * K + sk] != 0) {
    if (a.C > 0) {
      want = sc;
    } else {
      const long long c = a.det_cls[(long long)b * K + sk];
      want = (c >= 0 && c < IOU3D_EVAL_MAX_CLASS) ? (int)c : -2;
    }
  }
  double best = -INFINITY;
  int arg = -1;

  for (int g0 = 0; g0 < G; g0 += kMatchCols) {
    const int g = g0 + pg;
    const bool g_ok = g < G && a.gt_valid[(long long)b * G + g] != 0;
    if (pr == 0) {
      int c = -1;
      if (g_ok) {
        const long long v = a.gt_cls[(long long)b * G + g];
        c = (v >= 0 && v < IOU3D_EVAL_MAX_CLASS) ? (int)v : -1;
      }
      col_cls[pg] = c;
    }
    if (p_kept && g_ok) {
      float cg[24];
      load_box(a.gt + ((long long)b * G + g) * 24, cg);
      tile[pr][pg] = box3d_iou(cd, cg);
    }
    __syncthreads();
    if (want >= 0) {
      for (int j = 0; j < kMatchCols; ++j) {  // ascending g: the first maximum wins
        if (col_cls[j] == want) {
          const double v = tile[sr][j];
          if (v > best) { best = v; arg = g0 + j; }
        }
      }
    }
    __syncthreads();  // the next tile overwrites
  }
  if (s_live) {
    const long long o = ((long long)b * K + sk) * cm + sc;
    a.ovmax[o] = best;
    a.jmax[o] = arg;
  }
}

constexpr int kMarkThreads = 256;
constexpr int kMarkWaves = kMarkThreads / kWave;

__device__ __forceinline__ double mark_rec(int tp, long long npos) { return (double)tp / (double)npos; }

// tp / np.maximum(tp + fp, eps) (eval_det.py:150) at 0-based position `pos` of the class
__device__ __forceinline__ double mark_prec(int tp, long long pos) {
  const double tpd = (double)tp, fpd = (double)(pos + 1 - tp);
  return tpd / fmax(tpd + fpd, DBL_EPSILON);
}

__global__ __launch_bounds__(kMarkThreads)
void eval_mark_kernel(const EvalMarkArgs a) {
  __shared__ int wave_tp[kMarkWaves];
  __shared__ double sh[kMarkThreads];
  const int t = threadIdx.x, c = blockIdx.x, th = blockIdx.y;
  long long s0 = a.seg[c], s1 = a.seg[c + 1];
  if (s0 < 0 || s1 > a.n || s1 < s0) s0 = s1 = 0;  // a malformed segment table reads nothing
  const long long o = (long long)th * a.num_class + c;
  if (s1 == s0) {  // a class without detections: 0 / 0 / 0 (eval_det_multiprocessing :257-261)
    if (t == 0) { a.ap[o] = 0.0; a.last_rec[o] = 0.0; }
    return;
  }
  const double thr = a.thresh[th];
  const long long npos = a.npos[c];
  int *first = a.first + (long long)th * a.num_gt;
  int *ctp = a.cum_tp + (long long)th * a.n;

  // the first detection, in rank order, to claim each ground-truth box (eval_det.py:137-146)
  for (long long i = s0 + t; i < s1; i += kMarkThreads) {
    if (a.ovmax[i] > thr) {
      const int gid = a.gt_id[i];
      if (gid >= 0 && gid < a.num_gt) atomicMin(first + gid, (int)i);
    }
  }
  __syncthreads();

  // tp / fp prefix sums, rec and prec (eval_det.py:148-150)
  int carry = 0;
  for (long long base = s0; base < s1; base += kMarkThreads) {
    const long long i = base + t;
    int tp = 0;
    if (i < s1 && a.ovmax[i] > thr) {
      const int gid = a.gt_id[i];
      if (gid >= 0 && gid < a.num_gt &&
          __hip_atomic_load(first + gid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)i)
        tp = 1;
    }
    const unsigned long long m = __ballot(tp);
    int cum = mask_rank(m) + tp;
    if (lane_id() == 0) wave_tp[t / kWave] = __popcll(m);
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int w = 0; w < kMarkWaves; ++w) {
      if (w < t / kWave) cum += wave_tp[w];
      total += wave_tp[w];
    }
    cum += carry;
    carry += total;
    if (i < s1) {
      ctp[i] = cum;
      if (a.rec != nullptr) {
        a.rec[(long long)th * a.n + i] = mark_rec(cum, npos);
        a.prec[(long long)th * a.n + i] = mark_prec(cum, i - s0);
      }
    }
    __syncthreads();  // wave_tp is rewritten by the next chunk; ctp is read across lanes below
  }

  // voc_ap (eval_det.py:46-60): mrec = [0, rec, 1], mpre = [0, prec, 0], the envelope from the
  // right, the sum over the positions where mrec changes -- chunks from the last to the first
  const long long chunks = (s1 - s0 + kMarkThreads - 1) / kMarkThreads;
  double env_carry = 0.0, acc = 0.0;  // mpre's trailing 0; acc is thread 0's
  for (long long ch = chunks - 1; ch >= 0; --ch) {
    const long long i = s0 + ch * kMarkThreads + t;
    const bool live = i < s1;
    const int tp = live ? ctp[i] : 0;
    double env = live ? mark_prec(tp, i - s0) : 0.0;
    sh[t] = env;
    __syncthreads();
    for (int d = 1; d < kMarkThreads; d <<= 1) {  // suffix maximum of the chunk
      const double other = t + d < kMarkThreads ? sh[t + d] : 0.0;
      __syncthreads();
      env = fmax(env, other);
      sh[t] = env;
      __syncthreads();
    }
    const double chunk_max = sh[0];
    env = fmax(env, env_carry);
    env_carry = fmax(env_carry, chunk_max);
    double term = 0.0;
    if (live) {
      const double r = mark_rec(tp, npos);
      const double prev = i == s0 ? 0.0 : mark_rec(ctp[i - 1], npos);
      if (r != prev) term = (r - prev) * env;
    }
    __syncthreads();
    sh[t] = term;
    __syncthreads();
    for (int d = kMarkThreads / 2; d > 0; d >>= 1) {
      if (t < d) sh[t] += sh[t + d];
      __syncthreads();
    }
    if (t == 0) acc += sh[0];
    __syncthreads();
  }
  if (t == 0) {
    const double last = mark_rec(ctp[s1 - 1], npos);
    if (1.0 != last) acc += (1.0 - last) * 0.0;  // mrec's trailing 1 against mpre's trailing 0
    a.ap[o] = acc;
    a.last_rec[o] = last;
  }
}

}  // namespace

extern "C" __attribute__((visibility("default")))
int iou3d_eval_match(const EvalMatchArgs *args, void *stream) {
  if (args == nullptr) return (int)hipErrorInvalidValue;
  const EvalMatchArgs a = *args;
  if (a.C < 0 || a.C > IOU3D_EVAL_MAX_CLASS || a.G < 0 || a.K < 1 || a.B < 0 || a.B > 65535)
    return (int)hipErrorInvalidValue;
  if (a.B == 0) return 0;
  if (a.det == nullptr || a.keep == nullptr || a.ovmax == nullptr || a.jmax == nullptr ||
      (a.C == 0 && a.det_cls == nullptr) ||
      (a.G > 0 && (a.gt == nullptr || a.gt_valid == nullptr || a.gt_cls == nullptr)))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(eval_match_kernel, dim3((a.K + kMatchRows - 1) / kMatchRows, a.B),
                     dim3(kMatchThreads), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

extern "C" __attribute__((visibility("default")))
int iou3d_eval_mark(const EvalMarkArgs *args, void *stream) {
  if (args == nullptr) return (int)hipErrorInvalidValue;
  const EvalMarkArgs a = *args;
  if (a.n < 0 || a.n > 0x7fffffffLL || a.num_class < 1 || a.num_class > IOU3D_EVAL_MAX_CLASS ||
      a.num_thresh < 1 || a.num_thresh > 65535 || a.num_gt < 0 || a.num_gt > 0x7fffffffLL)
    return (int)hipErrorInvalidValue;
  if (a.seg == nullptr || a.npos == nullptr || a.thresh == nullptr || a.ap == nullptr ||
      a.last_rec == nullptr || (a.rec == nullptr) != (a.prec == nullptr) ||
      (a.n > 0 && (a.ovmax == nullptr || a.gt_id == nullptr || a.cum_tp == nullptr)) ||
      (a.num_gt > 0 && a.first == nullptr))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(eval_mark_kernel, dim3(a.num_class, a.num_thresh), dim3(kMarkThreads), 0,
                     (hipStream_t)stream, a);
  return (int)hipGetLastError();
}
