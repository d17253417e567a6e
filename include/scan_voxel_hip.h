/* scan_voxel_hip.h -- C ABI of the voxel-grid downsample of scan stores (csrc/scan_voxel.hip): one row
 * per occupied cell of an absolute grid, chosen on the device (votenet/scan_voxels.py:VoxelStore).
 *
 * The reference has no counterpart: its datasets are downsampled before they are stored.  Every
 * argument record is a HOST struct of device pointers handed to the kernels by value, as in
 * scan_tile_hip.h.
 *
 * The cell of a row with finite float32 coordinates p is c_a = floor(double(p_a) / v_a) per axis a, an
 * IEEE float64 division: the grid is anchored at the origin, -0.0 and +0.0 are cell 0, a coordinate on a
 * face belongs to the upper cell.  A row with some |c_a| >= 2^20 is OUT OF RANGE: it is counted per scan
 * and takes no further part.  The cell's key is ((c_z + 2^20) << 42) | ((c_y + 2^20) << 21) | (c_x + 2^20),
 * a 63-bit word.  A cell keeps the row with the smallest RANK:
 *   nearest == 0   the row's index in its scan;
 *   nearest != 0   (bits(float32(d2)) << 32) | index, d2 = (d_x d_x + d_y d_y) + d_z d_z in float64, not
 *                  contracted, rounded once, d_a = double(p_a) - (double(c_a) + 0.5) * v_a.
 * Scans never interact: equal cells of two scans are different cells.
 *
 * The table.  Scan s owns scene_scan_voxel_slots(count[s]) slots of the scratch from slot
 * slot_offset[s] on: a power of two >= 2 * count[s], so an open-addressing table of the scan's cells is
 * never more than half full and a linear probe always ends.  A slot is a 64-bit key word (all ones:
 * empty, which no key equals) and a 64-bit best word; the scratch is `total_slots` key words followed
 * by `total_slots` best words.  A run that does not lie inside [0, total_slots) is not touched: its
 * scan's rows are counted as out of range.
 */
#ifndef SCAN_VOXEL_HIP_H
#define SCAN_VOXEL_HIP_H

#include <stddef.h>

#include "scan_tile_hip.h" /* SCAN_TILE_SEGMENT, SCAN_TILE_BLOCK */

#ifdef __cplusplus
extern "C" {
#endif

#define SCAN_VOXEL_CELL_LIMIT (1 << 20) /* |c_a| < this */

/* The slots of the table of a scan of `count` rows: the smallest power of two >= 2 * count, at least 2.
 * A host function; 0 where count < 1 or count >= 2^30. */
long long scene_scan_voxel_slots(int count);

typedef struct ScanVoxelArgs {
  int S;                        /* scans in the store, <= 65535 */
  int C;                        /* columns of the raw rows: 3 or 6 */
  int max_segments;             /* ceil(largest count / SCAN_TILE_SEGMENT) */
  int nearest;                  /* 0: keep the first row of a cell; else the one nearest its centre */
  double voxel[3];              /* v_x, v_y, v_z in metres: finite, > 0 */
  long long total_slots;        /* slots of the scratch: the sum of the scans' runs */
  size_t scratch_bytes;         /* the size of `scratch`, >= 16 * total_slots */
  const float *cloud;           /* (P, C) raw rows of every scan */
  const long long *offset;      /* (S,) first row of each scan */
  const int *count;             /* (S,) rows of each scan, 1 <= count < 2^30 */
  const long long *slot_offset; /* (S,) first slot of each scan's run */
  void *scratch;                /* the table, 8-byte aligned */
  int *slot;                    /* (P,) per row: its cell's slot within the scan's run, -1 out of range */
  int *outside;                 /* (S,) per scan: its rows out of range */
} ScanVoxelArgs;

/* Two launches.  CLEAR: every key and best word of the scratch to all ones, `outside` to 0.  INSERT, one
 * thread per row: the row's cell; hash of the key (any 64-bit mixer: no result depends on it), linear
 * probe that claims a slot with a 64-bit compare-and-swap on the key word -- the slot is the row's where
 * the swap returns empty or the row's own key -- then a 64-bit minimum of the rank on the slot's best
 * word, and the slot written to `slot`.  Inside the launch the table is touched only through agent-scope
 * atomics and the probe compares what the swap returned.  The set of keys and each cell's minimum do not
 * depend on the order of the threads; the slots do.  The scratch, `slot` and `outside` may arrive
 * holding anything: every word a later launch reads is written here.
 * hipErrorInvalidValue, without a launch: NULL args or pointer, S outside 1..65535, C not 3 or 6,
 * max_segments < 1, a voxel size that is not finite and > 0, total_slots < 1, a scratch that is
 * misaligned or smaller than 16 * total_slots bytes. */
int scene_scan_voxel_mark(const ScanVoxelArgs *args, void *stream);

typedef struct ScanVoxelCountArgs {
  ScanVoxelArgs mark; /* as given to scene_scan_voxel_mark, which has run */
  int *counts;        /* (S, max_segments) out: kept rows of segment g of scan s */
} ScanVoxelCountArgs;

/* One launch, one workgroup per (scan, segment of SCAN_TILE_SEGMENT rows): row r is KEPT iff
 * slot[r] >= 0 and the best word of its slot equals its own rank.  Every entry of `counts` is written
 * (0 for a segment past the scan's rows); plain loads, one integer LDS atomic per wave.
 * hipErrorInvalidValue, without a launch: as scene_scan_voxel_mark, or counts NULL. */
int scene_scan_voxel_count(const ScanVoxelCountArgs *args, void *stream);

typedef struct ScanVoxelGatherArgs {
  ScanVoxelArgs mark;    /* as given to scene_scan_voxel_mark, which has run */
  long long rows;        /* rows of `out` and `source`: nothing is written at or past it */
  const long long *base; /* (S, max_segments) row of `out` where segment g's kept rows of scan s begin */
  float *out;            /* (rows, C) out: the kept rows, all columns bit for bit */
  int *source;           /* (rows,) out: each kept row's index in its scan */
} ScanVoxelGatherArgs;

/* One launch, one workgroup per (scan, segment): scene_scan_tile_gather's stable compaction (ballot,
 * lane rank, a scan over the workgroup's waves, SCAN_TILE_BLOCK rows per step) of the kept rows, in
 * the scan's order, onto `base`.
 * hipErrorInvalidValue, without a launch: as scene_scan_voxel_mark, or rows < 1, or base, out or source
 * NULL. */
int scene_scan_voxel_gather(const ScanVoxelGatherArgs *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif
