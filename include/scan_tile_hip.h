/* scan_tile_hip.h -- C ABI of the tiled scan path (csrc/scan_tile.hip): scans larger than a room cut
 * into overlapping room-sized windows on the device (votenet/scan_tiles.py:TileStore) and the
 * per-window detections of votenet/detect.py merged into one set per scan (detect_tiled).
 *
 * The reference has no counterpart: its datasets hold room-sized scans only.  The grid of windows
 * and cores is a small float64 table made on the host (scan_tiles.tile_grid) from the bounds the
 * first entry point returns; every pass over points or detections is one of the launches below.
 * Every argument record is a HOST struct of device pointers handed to the kernels by value, as in
 * scan_hip.h.  All compares are float32 against float32 tables that may hold infinities; a window
 * or core is [lo, hi): lower bound inclusive, upper bound exclusive.
 */
#ifndef SCAN_TILE_HIP_H
#define SCAN_TILE_HIP_H

#include <stddef.h>

#include "scan_hip.h" /* SCAN_MAX_K */

#ifdef __cplusplus
extern "C" {
#endif

#define SCAN_TILE_SEGMENT 65536 /* rows of a parent scan that one workgroup counts / gathers */
#define SCAN_TILE_BLOCK 1024    /* threads of those workgroups: rows per step of their loops */
#define SCAN_TILE_MAX 4096      /* tiles per scan */

typedef struct ScanBoundsArgs {
  int S;                   /* scans in the store */
  int C;                   /* columns of the raw rows: 3 or 6 */
  int max_segments;        /* ceil(largest count / SCAN_TILE_SEGMENT) */
  const float *cloud;      /* (P, C) raw rows of every scan */
  const long long *offset; /* (S,) first row of each scan */
  const int *count;        /* (S,) rows of each scan, 1 <= count < 2^30 */
  float *partial;          /* (S, max_segments, 4) scratch: only a scan's own segments are written and read */
  float *bounds;           /* (S, 4) out: xmin, xmax, ymin, ymax */
} ScanBoundsArgs;

/* Two launches: per (segment, scan) the minimum and maximum of x and of y over the segment's rows,
 * then per scan the same over its segments.  fminf / fmaxf only, so the result is exact whatever
 * the order; where an extreme is a zero its sign is unspecified, as scene_scan_prepare's floor.
 * The rows must be finite (ScanStore refuses the others).
 * hipErrorInvalidValue, without a launch: NULL args or pointer, S < 1, C not 3 or 6,
 * max_segments < 1. */
int scene_scan_bounds(const ScanBoundsArgs *args, void *stream);

typedef struct ScanTileCountArgs {
  int T;                   /* tiles */
  int C;                   /* columns of the raw rows: 3 or 6 */
  int max_segments;        /* as ScanBoundsArgs */
  const float *cloud;      /* (P, C) the parents' rows */
  const long long *offset; /* (S,) */
  const int *count;        /* (S,) */
  const int *parent;       /* (T,) the scan of each tile */
  const float *window;     /* (T, 4) wlo_x, whi_x, wlo_y, whi_y */
  int *counts;             /* (T, max_segments) out: rows of segment g of the tile's parent inside the window */
} ScanTileCountArgs;

/* One launch, one workgroup per (tile, segment): the number of the parent's rows r in
 * [g * SCAN_TILE_SEGMENT, (g + 1) * SCAN_TILE_SEGMENT) with wlo_x <= x < whi_x && wlo_y <= y < whi_y.
 * Every entry of `counts` is written (0 for a segment past the parent's rows), so the table needs
 * no clear; integer LDS atomics only.
 * hipErrorInvalidValue, without a launch: NULL args or pointer, T < 1, C not 3 or 6,
 * max_segments < 1. */
int scene_scan_tile_count(const ScanTileCountArgs *args, void *stream);

typedef struct ScanTileGatherArgs {
  int T;                   /* tiles that are built */
  int C;                   /* columns: 3 or 6 */
  int max_segments;        /* as ScanBoundsArgs */
  long long rows;          /* rows of `crops`: nothing is written at or past it */
  const float *cloud;      /* (P, C) the parents' rows */
  const long long *offset; /* (S,) */
  const int *count;        /* (S,) */
  const int *parent;       /* (T,) */
  const float *window;     /* (T, 4) */
  const long long *base;   /* (T, max_segments) row of `crops` where segment g's rows of the tile begin:
                              the tile's first row plus scene_scan_tile_count's counts of its segments before g */
  float *crops;            /* (rows, C) out */
} ScanTileGatherArgs;

/* One launch, one workgroup per (tile, segment): the rows scene_scan_tile_count counted, copied bit
 * for bit, all C columns, in the parent's order -- a stable compaction (ballot and lane rank inside
 * a wave, a scan over the workgroup's waves, SCAN_TILE_BLOCK rows per step) onto `base`.
 * hipErrorInvalidValue, without a launch: NULL args or pointer, T < 1, C not 3 or 6,
 * max_segments < 1, rows < 1. */
int scene_scan_tile_gather(const ScanTileGatherArgs *args, void *stream);

typedef struct ScanMergeArgs {
  int S;                   /* parent scans */
  int K;                   /* rows per tile of the tile arena, <= SCAN_MAX_K */
  int NC;                  /* > 0: per-class scores; 0: one score per row */
  int cap;                 /* rows per scan of the merged arena */
  int max_tiles;           /* the most tiles any scan has: cap >= max_tiles * K */
  const int *first;        /* (S,) each scan's first tile */
  const int *tiles;        /* (S,) each scan's number of tiles, <= max_tiles */
  const float *core;       /* (T, 4) clo_x, chi_x, clo_y, chi_y */
  /* the tile arena (scene_detections_pack's planes, indexed by tile) */
  const int *count_in;     /* (T,) */
  const int *proposal_in;  /* (T, K) */
  const int *cls_in;       /* (T, K) */
  const float *score_in;   /* (T, K) or (T, K, NC) */
  const float *box_in;     /* (T, K, 7) */
  const float *corners_in; /* (T, K, 8, 3) */
  /* the merged arena, indexed by scan */
  int *count;              /* (S,) owned rows of the scan */
  int *tile;               /* (S, cap) the tile (row of the tile store) a row came from */
  int *proposal;           /* (S, cap) */
  int *cls;                /* (S, cap) */
  float *score;            /* (S, cap) or (S, cap, NC) */
  float *box;              /* (S, cap, 7) */
  float *corners;          /* (S, cap, 8, 3) */
} ScanMergeArgs;

/* One launch, one workgroup per parent scan: the scan's tiles in store order, each tile's packed
 * rows in packed order (objectness descending); a row is owned iff its box centre has
 * clo_x <= x < chi_x && clo_y <= y < chi_y for the tile's core, and the owned rows are written
 * compacted, in that order, into the scan's rows of the merged arena; rows past `count` are zero,
 * so the arena needs no clear.  Reads the tile arena where the pack launches left it: no host copy.
 * hipErrorInvalidValue, without a launch: NULL args or pointer, S < 1, K outside 1..SCAN_MAX_K,
 * NC < 0, max_tiles < 1, cap < max_tiles * K. */
int scene_detections_merge(const ScanMergeArgs *args, void *stream);

#define SCAN_SEAM_PARTNERS 4 /* higher-ordered partners a row records; a row with more rescans its neighbours */

typedef struct ScanSeamArgs {
  int S;                   /* parent scans */
  int K;                   /* rows per tile of the tile arena, <= SCAN_MAX_K */
  int NC;                  /* > 0: per-class scores; 0: one score per row */
  int cap;                 /* rows per scan of the merged arena */
  int max_tiles;           /* the most tiles any scan has, <= SCAN_TILE_MAX: cap >= max_tiles * K */
  const int *first;        /* (S,) each scan's first tile */
  const int *tiles;        /* (S,) each scan's number of tiles, <= max_tiles */
  const float *core;       /* (T, 4) clo_x, chi_x, clo_y, chi_y */
  /* the tile arena, as ScanMergeArgs */
  const int *count_in;     /* (T,) */
  const int *proposal_in;  /* (T, K) */
  const int *cls_in;       /* (T, K) */
  const float *score_in;   /* (T, K) or (T, K, NC) */
  const float *box_in;     /* (T, K, 7) */
  const float *corners_in; /* (T, K, 8, 3) */
  /* the merged arena, as ScanMergeArgs; count: the scan's kept rows */
  int *count;              /* (S,) */
  int *tile;               /* (S, cap) */
  int *proposal;           /* (S, cap) */
  int *cls;                /* (S, cap) */
  float *score;            /* (S, cap) or (S, cap, NC) */
  float *box;              /* (S, cap, 7) */
  float *corners;          /* (S, cap, 8, 3) */
  /* the seam */
  const int *iy;           /* (T,) the tile's row in its scan's grid */
  const int *ix;           /* (T,) the tile's column */
  const float *reach;      /* (T, 4) rlo_x, rhi_x, rlo_y, rhi_y: the core grown by the seam width on its finite sides */
  double thresh;           /* two rows are partners where their overlap is > thresh */
  int old_type;            /* overlap = intersection / area of the lower-ordered row, not / union */
  int same_class;          /* rows of different classes never overlap; dims == 3 only */
  int dims;                /* 3: volumes of the bounds; 2: areas of their camera x / z footprint */
  void *scratch;           /* scene_detections_merge_nms_scratch_bytes(S, T, K, max_tiles) bytes, 8-byte aligned */
  size_t scratch_bytes;    /* the size of `scratch` */
} ScanSeamArgs;

/* The size of ScanSeamArgs.scratch for S scans of T tiles in all, K rows per tile, at most max_tiles
 * tiles per scan: per row of (scan, tile of the scan, packed row) the flags, the key, six float32
 * bounds, the float64 area, the partner counts, SCAN_SEAM_PARTNERS partner rows and the state of the
 * resolve.  A host function; 0 where an argument is < 1.  (T does not enter today: the rows are
 * addressed by scan and tile of the scan, so that the launches stay inside the buffer whatever
 * `first` holds.) */
size_t scene_detections_merge_nms_scratch_bytes(int S, int T, int K, int max_tiles);

/* scene_detections_merge with an NMS across the cuts: one box per object that two neighbouring tiles
 * both see.  Four launches, none of which waits on another workgroup:
 *   rows      per (scan, tile, 256 rows): row r < count_in is a CANDIDATE iff its box centre lies in the
 *             tile's reach (the four compares above), OWNED iff it lies in the core, else a GUEST; its
 *             bounds are the min / max of its eight corners per axis, its area / volume their float64
 *             product ((x2 - x1) * (y2 - y1)) * (z2 - z1), or (x2 - x1) * (z2 - z1) for dims == 2, its key
 *             score[row] (NC == 0) or score[row, cls[row]].
 *   partners  per candidate: the candidates of the other tiles of its scan with |iy - iy'| <= 1 and
 *             |ix - ix'| <= 1 whose overlap with it is > thresh -- float64, intersection l * w * h (l * h
 *             for dims == 2) of the clamped extents, / (area_hi + area_lo - intersection), or / area_lo with
 *             old_type, times (cls == cls') with same_class; 0 / 0 compares false.  It counts them and
 *             records the first SCAN_SEAM_PARTNERS that are ordered above it: key descending, then tile,
 *             then packed row ascending.  A candidate with none above it is a WINNER at once.
 *   resolve   one workgroup per scan, in rounds: a candidate loses as soon as a partner above it has
 *             won in an earlier round and wins once all of them have lost -- the greedy NMS in that
 *             order.  Every round decides the highest undecided row, so the loop is a `for` over at
 *             most the undecided rows; a row with more partners above it than it recorded rescans.
 *   write     scene_detections_merge's compaction with KEPT in place of owned: an owned winner, or a
 *             guest that won and has at least one partner.  Same layout, rows past `count` zero.
 * Rows of one tile never interact.  The scratch may arrive uninitialised: every word is written
 * before it is read.
 * hipErrorInvalidValue, without a launch: NULL args or pointer, S < 1, K outside 1..SCAN_MAX_K,
 * NC < 0, max_tiles outside 1..SCAN_TILE_MAX, cap < max_tiles * K, dims not 2 or 3, dims == 2 with
 * same_class, a scratch that is misaligned or smaller than the size above. */
int scene_detections_merge_nms(const ScanSeamArgs *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif
