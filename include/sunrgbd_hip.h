/* sunrgbd_hip.h -- C ABI of the SUN RGB-D batch builder (csrc/sunrgbd_batch.hip).
 *
 * A batch is built from a RESIDENT scene store (every scan's cloud, its oriented-box table and,
 * optionally, its (n, 10) vote rows packed once into device memory,
 * votenet/sunrgbd_data.py:SunRgbdScenes) with
 * the semantics of the reference's loaders (sunrgbd/sunrgbd_detection_dataset.py,
 * sunrgbd/sunrgbd_ssl_dataset.py): point sampling, flip-x / rotz(+-30 deg) / isotropic scale of the
 * student cloud, the per-point colour augmentation of the detection dataset, oriented-box labels
 * (heading through pi - theta, theta - rot_angle and angle2class; size residuals from 2 x the
 * half sizes), and the votes carried through the same flip, rotation and scale.  The vote rows
 * are either input data (the reference's extraction wrote them) or, when the store holds none,
 * computed per sampled point from the boxes by the extraction's own rule
 * (sunrgbd/sunrgbd_data.py:232-257); scene_sunrgbd_votes computes them for the whole store.  Every
 * random draw is the counter-based hash of scene_hip.h; per-point colour draws are keyed by the
 * SOURCE point index.  The struct travels by value; nothing is copied host -> device per batch.
 */
#ifndef SUNRGBD_HIP_H
#define SUNRGBD_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define SUN_MAX_B 64     /* scenes per batch */
#define SUN_MAX_OBJ 64   /* box rows per scene (MAX_NUM_OBJ) */
#define SUN_BOX_COLS 8   /* cx, cy, cz, l/2, w/2, h/2, heading, class */
#define SUN_VOTE_COLS 10 /* mask, three votes */

/* draw indices of the hash */
enum { SUN_DRAW_STUDENT = 0, SUN_DRAW_EMA = 1, SUN_DRAW_FLIP = 2, SUN_DRAW_ANGLE = 3,
       SUN_DRAW_SCALE = 4, SUN_DRAW_COLOR = 5 /* .. 10: brightness rgb, shift rgb */,
       SUN_DRAW_JITTER = 11, SUN_DRAW_DROP = 12 /* per point: element(key, source index) */ };

typedef struct SunBatchArgs {
  int B;              /* scenes (rows) in the batch, <= SUN_MAX_B */
  int N;              /* points per scene */
  int C;              /* channels of the stored cloud: xyz, [rgb - 0.5], [height] */
  int has_height;     /* the last channel is the height (scaled with the cloud) */
  int augment;        /* student cloud: flip / rotate / scale (training) */
  int color_aug;      /* the detection dataset's colour augmentation (needs C >= 6) */
  int ema;            /* also draw ema_point_clouds: an independent, un-augmented sample */
  int vote_rows;      /* rows [0, vote_rows) get vote labels */
  int box_rows;       /* rows [0, box_rows) get box labels */
  int box_aug_rows;   /* of those, rows [0, box_aug_rows) in the student (augmented) frame */
  int div256_from;    /* rows [div256_from, B): colour channels / 256 (the unlabeled dataset) */
  int NS;             /* size clusters of mean_size */
  int num_heading_bin;
  int u_point_stride; /* n_max of u_point_in */
  unsigned seed, counter;
  int scene[SUN_MAX_B];      /* store row of each batch row */
  int scan_idx[SUN_MAX_B];   /* written to scan_idx (the index in the row's own scan list) */
  int supervised[SUN_MAX_B]; /* written to supervised_mask */
  /* the resident store (device pointers) */
  const float *cloud;          /* (P, C) */
  const float *votes;          /* (P, SUN_VOTE_COLS); NULL: computed from boxes / nbox */
  const long long *offset;     /* (S,) first point of each scene */
  const int *count;            /* (S,) points of each scene (>= 1) */
  const double *boxes;         /* (S, SUN_MAX_OBJ, SUN_BOX_COLS) */
  const int *nbox;             /* (S,) */
  const double *mean_size;     /* (NS, 3) */
  /* explicit draws (parity tests); NULL: draw on the device */
  const int *idx_in;           /* (B, N) student sample, in [0, count) */
  const int *ema_idx_in;       /* (B, N) teacher sample */
  const double *u_in;          /* (B, 3) uniforms in [0,1): flip, angle, scale */
  const double *u_color_in;    /* (B, 6) brightness rgb, shift rgb */
  const double *u_point_in;    /* (B, 2, u_point_stride) jitter, drop by source point index */
  /* outputs (data.make_batch / make_semi_batch keys); NULL: not written */
  float *point_clouds;         /* (B, N, C) */
  float *ema_point_clouds;     /* (B, N, C) */
  float *vote_label;           /* (vote_rows, N, 9) */
  long long *vote_label_mask;  /* (vote_rows, N) */
  float *center_label;         /* (box_rows, 64, 3) */
  long long *heading_class_label; /* (box_rows, 64) */
  float *heading_residual_label;  /* (box_rows, 64) */
  long long *size_class_label;    /* (box_rows, 64) */
  float *size_residual_label;     /* (box_rows, 64, 3) */
  long long *sem_cls_label;       /* (box_rows, 64) */
  float *box_label_mask;          /* (box_rows, 64) */
  long long *supervised_mask;  /* (B,) */
  long long *scan_idx_out;     /* (B,) */
  long long *flip_x_axis, *flip_y_axis; /* (B,) */
  float *rot_angle;            /* (B,) */
  float *rot_mat;              /* (B, 3, 3) */
  float *scale;                /* (B, 1, 3) */
} SunBatchArgs;

/* Build one batch: two launches on `stream` (draws + box labels; sample + gather + augment +
 * votes).  `args` is a HOST struct of device pointers. */
int scene_sunrgbd_batch_build(const SunBatchArgs *args, void *stream);

/* The vote rows of a whole store from its boxes: sunrgbd/sunrgbd_data.py:232-257 (the vote loop of
 * extract_sunrgbd_data(save_votes=True)) with the membership test of sunrgbd/sunrgbd_utils.py:215-237
 * (the hull of my_compute_box_3d's corners, i.e. the oriented box).  For point p (float32) of scene
 * s and its box rows k = 0 .. nbox[s]-1 in table order, in float64: d = p - centre, lx = d.x cos t -
 * d.y sin t, ly = d.x sin t + d.y cos t; p is inside iff |lx| <= |l|, |ly| <= |w|, |d.z| <= |h|; a
 * box with a zero half size contains nothing (its hull is flat: the extraction skips the object).
 * The first containing box sets the mask and writes (float)(centre - p) to all three vote slots,
 * the second to slot 1, the third and every later one to slot 2.  A point in no box gets ten zeros.
 *   cloud (P, C) float32 with C >= 3; offset / count (scenes,): the rows of each scene; boxes
 *   (scenes, SUN_MAX_OBJ, SUN_BOX_COLS) float64; votes_out (P, SUN_VOTE_COLS) float32.
 * One launch on `stream`.  hipErrorInvalidValue, and nothing launched, for a NULL pointer, C < 3,
 * scenes < 1 or scenes > 65535 (the grid's second dimension). */
int scene_sunrgbd_votes(const float *cloud, int C, const long long *offset, const int *count,
                        const double *boxes, const int *nbox, int scenes, float *votes_out,
                        void *stream);

#ifdef __cplusplus
}
#endif
#endif
