/* sunrgbd_raw_hip.h -- C ABI of the raw SUN RGB-D export (csrc/sunrgbd_raw.hip;
 * votenet/sunrgbd_raw.py holds the readers, the box table and the numpy restatement).
 *
 * What the reference does per scene in sunrgbd/sunrgbd_data.py:225-229 (the subsample of the depth
 * cloud to num_point rows) and what votenet/sunrgbd_data.read_scene does with the saved rows (rgb -
 * 0.5, the floor np.percentile(z, 0.99), height = z - floor, one rounding to float32), for a CHUNK of
 * scenes of ONE element type in flat arrays with an offset table.  The box table comes from the
 * label files on the host (at most 64 rows a scene) and the vote rows from scene_sunrgbd_votes.
 * The host has validated every index a kernel follows: explicit choices against the point count.
 * The record is a HOST struct of device pointers handed to the kernels by value.
 */
#ifndef SUNRGBD_RAW_HIP_H
#define SUNRGBD_RAW_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

enum { SUNRAW_KEEP_DRAWN = 0, SUNRAW_KEEP_GIVEN = 1 };
enum { SUNRAW_FLOAT32 = 0, SUNRAW_FLOAT64 = 1 };
#define SUNRAW_ROW_COLS 7 /* a store row: x y z, r g b - 0.5, z - floor */

typedef struct SunRgbdRawArgs {
  int S;         /* scenes of the chunk, >= 1 */
  int num_point; /* kept rows of every scene, >= 1; S * num_point < 2^31 */
  int elem;      /* SUNRAW_FLOAT32 / SUNRAW_FLOAT64: the element type of raw, kept and floor */
  unsigned seed; /* drawn choices: draw (seed, 0, scan_index, SB_DRAW_STUDENT) of csrc/scene_common.h */
  long long P;   /* raw rows of the chunk, S <= P < 2^31 */
  /* the chunk (device pointers) */
  const void *raw;             /* (P, 6) x y z r g b as the depth file has them */
  const long long *raw_offset; /* (S + 1,) first raw row of each scene; [S] = P; 1 <= rows of a scene < 2^30 */
  const int *keep;             /* (S,) SUNRAW_KEEP_*: num_point rows drawn, or given */
  const int *scan_index;       /* (S,) the scene's place in the whole export: the row of its draw */
  const int *choice;           /* (S * num_point,) the kept raw row of each slot of a SUNRAW_KEEP_GIVEN scene */
  /* outputs */
  void *kept;     /* (S * num_point, 6) the kept raw rows, element type `elem` */
  void *floor;    /* (S,) np.percentile(kept z, 0.99) in `elem` */
  unsigned long long *nonfinite; /* (S,) NaN and Inf among ALL raw values of each scene */
  float *rows;    /* (S * num_point, SUNRAW_ROW_COLS) the store rows */
} SunRgbdRawArgs;

/* Three launches on `stream`.  (1) one thread per kept slot, workgroups straddling scene boundaries:
 * the slot's raw row (the draw, or `choice`), copied.  (2) one workgroup per scene: the floor of the
 * kept z -- the two order statistics of numpy's linear method selected exactly by 8-bit radix passes
 * over the order-preserving integer image of z (four passes for float32, eight for float64), numpy's
 * lerp in `elem`, every operation rounded -- and the scene's cleared count.  (3) one thread per kept
 * slot and per raw row: the store row, arithmetic in `elem`, one rounding to float32; the raw row's
 * non-finite values, added to its scene's count by integer atomics (none in a sound chunk).
 * hipErrorInvalidValue, without a launch: NULL args or pointer, S < 1, num_point < 1, S * num_point
 * above 2^31-1, P outside S..2^31-1, an unknown `elem`. */
int scene_sunrgbd_raw_export(const SunRgbdRawArgs *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif
