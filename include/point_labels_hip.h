/* point_labels_hip.h -- C ABI of the per-point instance labels of packed detections
 * (csrc/point_labels.hip): which packed row owns each raw row of a scan store
 * (votenet/point_labels.py:label_points, whose docstring states the rule once).
 *
 * The reference answers the question with extract_pc_in_box3d (sunrgbd/sunrgbd_utils.py:215-224), a
 * scipy Delaunay hull per box on the host.  Here membership is csrc/box_points.hip's closed-form test,
 * transposed: one lane per POINT, the boxes staged through LDS.  Every argument record is a HOST
 * struct of device pointers handed to the kernels by value, as in scan_voxel_hip.h.
 *
 * The detections are read through four planes of a packed arena (include/scan_hip.h,
 * include/scan_tile_hip.h), `cap` rows per scan: count (S,), cls (S, cap), score (S, cap) or
 * (S, cap, NC), box (S, cap, 7).  Either layout works.  Rows at or past min(max(count, 0), cap) are
 * never read.
 *
 * FRAME of row r from box = (cx, cy, cz, l, w, h, heading): c = float(cos(double(heading))),
 * s = float(sin(double(heading))), hl, hw, hh = float(double(size) / 2); eight floats
 * c, s, cx, cy, cz, hl, hw, hh.
 * KEY: score[r], or with NC > 0 score[r, cls[r]] (a cls outside [0, NC) makes the row ineligible).
 * ELIGIBLE: r < count, all eight frame values finite, l, w, h > 0, key not NaN and
 * double(key) >= max(min_score, 0).
 * RANK, a 64-bit word, 0 for an ineligible row; else the low word is 0xFFFFFFFF - r and the high word
 *   prefer == 0 (score)     bits(|key|)
 *   prefer == 1 (smallest)  0xFFFFFFFF - bits(v), v = (l * w) * h in float32, each product rounded.
 * INSIDE (float32, every operation rounded, no contraction): d = p - centre, x' = c dx - s dy,
 * z' = s dx + c dy; |x'| <= hl & |z'| <= hw & |dz| <= hh.
 * OWNER of a point: the eligible row containing it with the largest rank, else -1.
 *
 * The scratch is S * cap rank words (8 bytes each), then S * cap int32 cls, then S * cap float32
 * bounding radii: 16 * S * cap bytes, 8-byte aligned.
 */
#ifndef POINT_LABELS_HIP_H
#define POINT_LABELS_HIP_H

#include <stddef.h>

#include "scan_hip.h" /* SCAN_MAX_K */

#ifdef __cplusplus
extern "C" {
#endif

#define LABEL_BLOCK 256     /* points, and threads, per workgroup of scene_points_label */
#define LABEL_BOX_CHUNK 256 /* rows staged through LDS at a time */

/* Bytes of the scratch of S scans with cap rows each: 16 * S * cap; 0 where S < 1 or cap < 1.  A host
 * function. */
size_t scene_points_label_scratch_bytes(int S, int cap);

typedef struct DetectionsFramesArgs {
  int S;                /* scans, 1..65535 */
  int K;                /* proposals per detector pass, 1..SCAN_MAX_K (cap is a multiple of it) */
  int cap;              /* rows per scan of the planes, >= 1 */
  int NC;               /* 0: one score per row; else scores per row */
  int prefer;           /* 0: score, 1: smallest */
  double min_score;     /* finite */
  const int *count;     /* (S,) */
  const int *cls;       /* (S, cap) */
  const float *score;   /* (S, cap) or (S, cap, NC) */
  const float *box;     /* (S, cap, 7) */
  float *frames;        /* (S, cap, 8) out: the frame of every row < count, zeros past it */
  int *points;          /* (S, cap) out: zeroed */
  void *scratch;        /* out: rank, cls, radius of every row (0, 0, 0 past count) */
  size_t scratch_bytes; /* >= scene_points_label_scratch_bytes(S, cap) */
} DetectionsFramesArgs;

/* One launch, one thread per (scan, row < cap).  Every word of frames, points and the first
 * 16 * S * cap bytes of the scratch is written, so all of them may arrive holding anything.  The
 * radius of an eligible row is an upper bound, inflated by 2^-10, of the distance from its centre of
 * any point the float32 test can accept (sqrt(hl^2 + hw^2 + hh^2) in float64, rounded up).
 * hipErrorInvalidValue, without a launch: NULL args or pointer, S outside 1..65535, K outside
 * 1..SCAN_MAX_K, cap < 1, NC < 0, prefer outside {0, 1}, min_score not finite, a scratch that is
 * misaligned or too small. */
int scene_detections_frames(const DetectionsFramesArgs *args, void *stream);

typedef struct PointsLabelArgs {
  int S;                   /* scans of the store == scans of the detections, 1..65535 */
  int C;                   /* columns of the raw rows: 3 or 6 */
  int K;                   /* as in DetectionsFramesArgs */
  int cap;                 /* rows per scan, >= 1 */
  int cull;                /* != 0: drop a staged row whose bounding sphere misses the workgroup's points */
  int max_blocks;          /* ceil(largest count / LABEL_BLOCK), >= 1 */
  const float *cloud;      /* (P, C) raw rows of every scan */
  const long long *offset; /* (S,) first row of each scan */
  const int *count;        /* (S,) rows of each scan */
  const int *rows;         /* (S,) the detections' count plane */
  const float *frames;     /* (S, cap, 8) as scene_detections_frames wrote them */
  const void *scratch;     /* as scene_detections_frames wrote it */
  size_t scratch_bytes;
  int *instance;           /* (P,) out: the owner of every point, -1 for none */
  int *semantic;           /* (P,) out: cls of the owner, -1 for none */
  int *points;             /* (S, cap) in / out: += the points each row owns (zeroed by the frames launch) */
} PointsLabelArgs;

/* One launch, grid (max_blocks, S), LABEL_BLOCK threads: one lane per point with its xyz in
 * registers; the scan's eligible rows pass through LDS LABEL_BOX_CHUNK at a time (frame and rank,
 * compacted; every lane reads the same address) and the lane keeps the largest rank of the rows that
 * contain it.  With `cull` a row is staged only if its sphere (centre, radius) reaches the bounding
 * box of the workgroup's points, tested in float64: the result does not depend on it.  instance and
 * semantic are plain stores; points gets agent-scope integer atomic adds, equal owners of a wave
 * merged first.  No float atomics.
 * hipErrorInvalidValue, without a launch: NULL args or pointer, S outside 1..65535, C not 3 or 6, K
 * outside 1..SCAN_MAX_K, cap < 1, max_blocks < 1, a scratch that is misaligned or too small. */
int scene_points_label(const PointsLabelArgs *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif
