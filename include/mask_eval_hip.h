/* mask_eval_hip.h -- C ABI of the mask matching of per-point labels against ground-truth instances
 * (csrc/mask_eval.hip): for every packed detection the best point-set IoU with a ground-truth
 * instance of its class, in the form iou3d_eval_mark consumes (votenet/mask_eval.py:match_masks,
 * whose docstring states the rule once; MaskAPCalculator feeds the marking kernel with it).
 *
 * Every argument record is a HOST struct of device pointers handed to the kernels by value, as in
 * point_labels_hip.h.  Scan s has count[s] points, rows offset[s] .. offset[s] + count[s] of the flat
 * per-point arrays.
 *
 * PREDICTION per point: instance (the owning packed row, -1 none: scene_points_label's output); per
 * row points[s, r] (the points the row owns) and the planes count (S,), cls (S, cap), score (S, cap)
 * or (S, cap, NS) of the packed detections.  A row's SCORE is score[r], or with NS > 0
 * score[r, cls[r]].
 * TRUTH per point: truth_instance (1..G names an instance, <= 0 and > G none), truth_class (the
 * detector's class id 0..NC-1; anything else: not a class).
 *
 *   size[s, g]      points of scan s with truth_instance == g + 1, g in [0, G)
 *   class[s, g]     truth_class of that instance's lowest-index point (-1 where size is 0)
 *   eligible g      size >= min_truth_points and 0 <= class < NC
 *   inter[s, r, g]  points with instance == r (0 <= r < cap) and truth_instance == g + 1
 *   detection r     r < min(max(count[s], 0), cap) and points[s, r] >= min_points (>= 1) and
 *                   0 <= cls[s, r] < min(NC, 64)
 *   iou(r, g)       double(inter) / double(points[s, r] + size[s, g] - inter): one IEEE division
 *   ovmax[s, r]     the largest iou(r, g) over eligible g with class[s, g] == cls[s, r];
 *   jmax[s, r]      the lowest such g reaching it; (-inf, -1) where there is none or r is no detection
 *   npos[c]         eligible g of class c < 64; npos[64]: g with size >= min_truth_points and a
 *                   class outside [0, 64)
 *
 * Scans never interact.  A prediction's size counts all its points.  Everything up to the one
 * division is an integer: two runs are bit-equal.
 *
 * The scratch holds three tables: S * G 64-bit class words (point index << 32 | class bits, all
 * ones where the instance has no point), then S * G int32 sizes, then S * cap * G int32
 * intersections: 4 * S * G * (cap + 3) bytes, 8-byte aligned.
 */
#ifndef MASK_EVAL_HIP_H
#define MASK_EVAL_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MASK_BLOCK 256       /* points, and threads, per workgroup of scene_mask_overlap */
#define MASK_MERGE_ROUNDS 4  /* rounds of the in-wave merge per key; lanes left after them add alone */
#define MASK_MAX_CLASS 64    /* == IOU3D_EVAL_MAX_CLASS: class ids 0 .. 63 are reported */
#define MASK_MATCH_ROWS 4    /* rows, one wave each, per workgroup of scene_mask_match */

/* Bytes of the scratch: 4 * S * G * (cap + 3); 0 where S, cap or G < 1.  A host function. */
size_t scene_mask_scratch_bytes(int S, int cap, int G);

typedef struct MaskOverlapArgs {
  int S;                     /* scans, 1..65535 */
  int cap;                   /* rows per scan of the detections, >= 1 */
  int G;                     /* the largest truth instance id, >= 1; S * G * (cap + 3) <= 2^31 */
  int max_blocks;            /* ceil(largest count / MASK_BLOCK), >= 1 */
  int merge;                 /* != 0: equal keys of a wave merged before the atomic; 0: one atomic per lane */
  int clear;                 /* != 0: a launch that empties the three tables goes first */
  const long long *offset;   /* (S,) first point of each scan */
  const int *count;          /* (S,) points of each scan */
  const int *instance;       /* (P,) */
  const int *truth_instance; /* (P,) */
  const int *truth_class;    /* (P,) */
  void *scratch;             /* in / out: the three tables, added to */
  size_t scratch_bytes;      /* >= scene_mask_scratch_bytes(S, cap, G) */
} MaskOverlapArgs;

/* With `clear` one launch writes every word of the three tables (zeros; all ones for the class
 * words), so the scratch may arrive holding anything.  Then one launch, grid (max_blocks, S),
 * MASK_BLOCK threads, one lane per point, 12 bytes read per point: size[s, g] += 1, class word
 * [s, g] = min(itself, index << 32 | class bits), inter[s, r, g] += 1.  Integer agent-scope atomics
 * only; the tables are read by a later launch, so there is no fence in the kernel.
 * With `merge` the lanes of a wave that share a key are served by ONE atomic of their leader (ballot,
 * broadcast of the leader's key, popcount of the matching lanes), for at most MASK_MERGE_ROUNDS
 * distinct keys; the lanes still unserved then issue their own.  The rounds are entered only where at
 * least half of the wave's keyed lanes hold the key of the lane after them (runs, as a scan's rows have
 * them); a wave of scattered keys goes to per-lane atomics at once.  The size and class updates merge
 * on g in rounds of their own (the leader is the lowest lane of its g, so its own class word is the
 * least); the intersections then merge on (r, g).  Both forms give the same tables.
 * hipErrorInvalidValue, without a launch: NULL args or pointer, S outside 1..65535, cap, G or
 * max_blocks < 1, more than 2^31 table entries, a scratch that is misaligned or too small. */
int scene_mask_overlap(const MaskOverlapArgs *args, void *stream);

typedef struct MaskMatchArgs {
  int S, cap, G;
  int NC;                /* classes of the detector, >= 1 */
  int NS;                /* 0: one score per row; else scores per row */
  int min_points;        /* >= 1 */
  int min_truth_points;  /* >= 1 */
  const int *rows;       /* (S,) the detections' count plane */
  const int *cls;        /* (S, cap) */
  const float *score;    /* (S, cap) or (S, cap, NS) */
  const int *points;     /* (S, cap) points each row owns */
  const void *scratch;   /* as scene_mask_overlap left it */
  size_t scratch_bytes;
  double *ovmax;         /* (S, cap) out */
  int *jmax;             /* (S, cap) out */
  float *row_score;      /* (S, cap) out: the row's score, 0 where it is no detection */
  short *key;            /* (S, cap) out: cls, MASK_MAX_CLASS + 1 where it is no detection */
  int *klass;            /* (S, G) out: class[s, g] */
  long long *npos;       /* (MASK_MAX_CLASS + 1,) in / out: ADDED to */
} MaskMatchArgs;

/* One launch, one wave per (scan, row), MASK_MATCH_ROWS waves per workgroup.  The lanes stride over
 * g, each keeps its best (iou, lowest g), and a butterfly ordered by iou, then by lower g, leaves the
 * row's.  Every element of ovmax, jmax, row_score, key and klass is written (klass and npos by the
 * wave of row 0 of each scan); npos is added to with integer atomics, so an epoch accumulates.
 * hipErrorInvalidValue, without a launch: NULL args or pointer, S outside 1..65535, cap, G, NC,
 * min_points or min_truth_points < 1, NS < 0, more than 2^31 table entries, a scratch that is
 * misaligned or too small. */
int scene_mask_match(const MaskMatchArgs *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif
