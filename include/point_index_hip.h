/* point_index_hip.h -- C ABI of the per-detection point lists (csrc/point_index.hip): a stable
 * multi-split of every scan's rows by an integer key, on the device, bit-reproducible
 * (votenet/point_index.py:PointLabels.index, whose docstring states the rule once).
 *
 * The reference has no counterpart: it asks each box for its points again (extract_pc_in_box3d).  Here
 * the label plane of point_labels_hip.h is turned into CSR lists.  The argument record is a HOST struct
 * of device pointers handed to the kernels by value, as in point_labels_hip.h.
 *
 * For each scan s with n = count[s] rows, local row j has the key k_j = key[offset[s] + j] and the
 * BUCKET b_j = k_j if 0 <= k_j < cap, else cap (the tail: -1 and every out-of-range key; a key is
 * compared, never followed as an index).
 * ORDER: order[offset[s] .. offset[s] + n) is the permutation of 0..n-1 that sorts b stably: bucket 0's
 * rows in ascending index, then bucket 1's, ..., the tail last.
 * START: start[s, r] = #{j : b_j < r} for r = 0..cap, so row r's list is
 * order[offset[s] + start[s, r] .. offset[s] + start[s, r + 1]) and start[s, cap] is the owned total.
 *
 * An LSD radix split with digits of INDEX_DIGIT_BITS bits: cap <= 2^INDEX_DIGIT_BITS - 1 takes ONE
 * pass, larger ones two, up to INDEX_MAX_CAP (the merged layout's ceiling SCAN_TILE_MAX x SCAN_MAX_K is
 * 2^22).  A pass has D = min(2^INDEX_DIGIT_BITS, (cap >> shift) + 1) digits.  The scratch holds, in
 * this order,
 *   the table    S * max_segments * D0 int32 (D0: pass 0's digits): a row of digit counts, then
 *                cursors, per (scan, segment of INDEX_SEGMENT rows)
 *   the bases    S * D0 int32: per scan, each digit's total, then its first position
 *   three planes of P int32 each, ONLY with two passes: pass 0's buckets and indices, the sorted buckets
 * 8-byte aligned; bounded by the digit width, never segments x cap.
 */
#ifndef POINT_INDEX_HIP_H
#define POINT_INDEX_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define INDEX_DIGIT_BITS 13 /* 8192 LDS counters (32 KB) per workgroup */
#define INDEX_SEGMENT 4096  /* rows per workgroup of the count and scatter launches */
#define INDEX_TILE 256      /* rows, and threads, a workgroup places at a time */
#define INDEX_MAX_CAP ((1 << (2 * INDEX_DIGIT_BITS)) - 1) /* two digits */

/* Bytes of the scratch for S scans of at most max_segments * INDEX_SEGMENT rows each, P rows in all,
 * keys split into cap + 1 buckets; 0 where S < 1, cap outside 1..INDEX_MAX_CAP, max_segments < 1 or
 * P < 0.  A host function. */
size_t scene_points_index_scratch_bytes(int S, int cap, int max_segments, long long P);

typedef struct PointsIndexArgs {
  int S;                   /* scans, 1..65535 */
  int cap;                 /* buckets below the tail (rows per scan of the detections), 1..INDEX_MAX_CAP */
  int max_segments;        /* ceil(largest count / INDEX_SEGMENT), >= 1 */
  long long P;             /* rows of key and order: every offset[s] + count[s] <= P */
  const int *key;          /* (P,) flat over the scans */
  const long long *offset; /* (S,) first row of each scan */
  const int *count;        /* (S,) rows of each scan */
  int *start;              /* (S, cap + 1) out */
  int *order;              /* (P,) out: every row of every scan (rows of no scan are not written) */
  void *scratch;           /* out */
  size_t scratch_bytes;    /* >= scene_points_index_scratch_bytes(S, cap, max_segments, P) */
} PointsIndexArgs;

/* Per pass four launches -- count (grid (max_segments, S): digit counts in LDS with integer LDS
 * atomics, a table row out), segments (one thread per (scan, digit) runs down the scan's segments),
 * digits (one workgroup per scan: an exclusive scan over the digits; in a single pass this IS start),
 * scatter (grid (max_segments, S): the cursor row in LDS, the segment walked in order INDEX_TILE rows
 * at a time; equal digits of a wave are ranked by lane from ballots, the four waves of a tile take
 * the cursors in turn) -- and with two passes a ninth launch at the end that reads start off the
 * sorted buckets' boundaries.  No host read, no synchronising call, no allocation.  Integer LDS
 * atomics in the count launch only: no global atomics, no float atomics.  Every word of start, of the
 * scans' rows of order and of the scratch that is read is written first, so all three may arrive
 * holding anything; nothing is written behind them.  The result does not depend on the order in which
 * waves or workgroups run: it is bit-equal to votenet/point_index.py:host_point_index.  A count
 * below 0 is 0; rows past max_segments * INDEX_SEGMENT of a scan are not indexed.
 * hipErrorInvalidValue, without a launch: NULL args or pointer, S outside 1..65535, cap outside
 * 1..INDEX_MAX_CAP, max_segments < 1, P < 0, a scratch that is misaligned or too small. */
int scene_points_index(const PointsIndexArgs *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif
