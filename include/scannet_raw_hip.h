/* scannet_raw_hip.h -- C ABI of the raw-ScanNet export (csrc/scannet_raw.hip;
 * votenet/scannet_raw.py holds the readers, the seg tables and the numpy restatement).
 *
 * What the reference does per scan in Python dictionaries (scannet/load_scannet_data.py:60-129
 * export, scannet/batch_load_scannet_data.py:49-79 export_one_scan) -- the axis alignment, the
 * per-vertex instance and semantic ids, the per-object axis-aligned boxes, the 18-class filter and
 * the subsample to MAX_NUM_POINT -- for a CHUNK of scans in flat arrays with offset tables, laid out
 * like the stores.  The host has reduced the two JSON files to tables over segment ids
 * (scannet_raw.seg_tables) and has validated every index the kernels follow: segment ids against
 * their table, object ids against 1..objects, explicit choices against the vertex count.
 * The record is a HOST struct of device pointers handed to the kernels by value.
 */
#ifndef SCANNET_RAW_HIP_H
#define SCANNET_RAW_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define SNR_MAX_OBJECTS 1024 /* objects per scan (scannet_data.MAX_INSTANCES): one workgroup compacts them */

enum { SNR_KEEP_ALL = 0, SNR_KEEP_DRAWN = 1, SNR_KEEP_GIVEN = 2 };

typedef struct ScanNetRawArgs {
  int S;           /* scans of the chunk, >= 1 */
  long long P;     /* vertices of the chunk, S <= P < 2^31 */
  long long Q;     /* output rows of the chunk, S <= Q <= P */
  long long T;     /* objects of the chunk, >= 0 */
  int max_objects; /* the largest object count of a scan, <= SNR_MAX_OBJECTS */
  int max_points;  /* MAX_NUM_POINT: the slots of a drawn choice */
  unsigned seed;   /* drawn choices: draw (seed, 0, scan_index, SB_DRAW_STUDENT) of csrc/scene_common.h */
  /* the chunk (device pointers) */
  const float *raw;             /* (P, 6) x y z r g b as the mesh file has them */
  const int *seg;               /* (P,) segIndices, 0 <= seg < the scan's table length */
  const double *matrix;         /* (S, 16) axisAlignment, row major */
  const long long *vert_offset; /* (S + 1,) first vertex of each scan; [S] = P < 2^31 */
  const long long *seg_offset;  /* (S + 1,) first entry of each scan's seg tables */
  const int *seg_label;         /* nyu40 id of each segment, 0: unannotated */
  const int *seg_object;        /* objectId + 1 of each segment in 0..objects, 0: none */
  const long long *obj_offset;  /* (S + 1,) first object of each scan; [S] = T */
  const int *object_label;      /* (T,) nyu40 id of each object */
  const long long *out_offset;  /* (S + 1,) first output row of each scan; [S] = Q < 2^31 */
  const int *keep;              /* (S,) SNR_KEEP_*: every vertex in order, max_points drawn, or given */
  const int *scan_index;        /* (S,) the scan's place in the whole export: the row of its draw */
  const int *choice;            /* (Q,) the kept vertex of each output row of a SNR_KEEP_GIVEN scan */
  /* scratch */
  unsigned *extent;             /* (T, 6) integer images of min xyz, max xyz; initialised by the entry */
  /* outputs */
  float *vert;                  /* (Q, 6) aligned xyz, raw rgb */
  unsigned *ins_label;          /* (Q,) */
  unsigned *sem_label;          /* (Q,) */
  double *bbox;                 /* (T, 7) the kept boxes of scan s from row obj_offset[s] on */
  int *nbox;                    /* (S,) kept boxes of each scan */
} ScanNetRawArgs;

/* scannet/load_scannet_data.py:60-129 and scannet/batch_load_scannet_data.py:49-79 for a chunk of
 * scans, in launches on `stream`: the empty extents; one launch over the P vertices (the aligned
 * coordinate in float64, left to right and un-contracted, rounded to float32; the object's extents
 * from ALL vertices by integer atomic min / max on order-preserving images, reduced per wave first); one
 * workgroup per scan (centre and size in float32 as numpy computes them on float32 scalars, stored
 * as float64 with the object's label; the rows whose label is one of the 18 OBJ_CLASS_IDS, compacted
 * in object order); one launch over the Q output rows (the kept vertices' aligned xyz, raw rgb,
 * instance and semantic ids).
 * hipErrorInvalidValue, without a launch: NULL args or pointer (`choice` may be NULL), S < 1, P or Q
 * outside S..2^31-1, Q > P, T < 0, max_points < 1, max_objects outside 0..SNR_MAX_OBJECTS. */
int scannet_raw_export(const ScanNetRawArgs *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif
