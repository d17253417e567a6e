/* scene_hip.h -- C ABI of the ScanNet batch builder (csrc/scene_batch.hip).
 *
 * A batch is built from a RESIDENT scene store (every scan's points, labels and box table packed
 * once into device memory, votenet/scannet_data.py:ScanNetScenes) with the semantics of the
 * reference's loaders (scannet/scannet_ssl_dataset.py, scannet/scannet_detection_dataset.py):
 * point sampling (pc_util.random_sampling), flip-x / flip-y / rotz(+-5 deg) / isotropic scale of
 * the student cloud, box labels (rotate_aligned_boxes), and vote labels computed AFTER the
 * augmentation.  Every random draw is a counter-based hash of (seed, counter, batch row, draw
 * index), so a batch is a pure function of the arguments; scene ids and the counter travel in the
 * argument struct, which the launcher hands to the kernels by value (nothing is copied host ->
 * device per batch).
 */
#ifndef SCENE_HIP_H
#define SCENE_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define SB_MAX_B 64      /* scenes per batch */
#define SB_MAX_OBJ 64    /* box rows per scene (MAX_NUM_OBJ) */
#define SB_MAX_INST 1024 /* dense instance ids per scene */
#define SB_BOX_COLS 7    /* cx, cy, cz, dx, dy, dz, class index */

/* draw indices of the hash (the order the reference draws in does not matter on the device) */
enum { SB_DRAW_STUDENT = 0, SB_DRAW_EMA = 1, SB_DRAW_FLIP_X = 2, SB_DRAW_FLIP_Y = 3,
       SB_DRAW_ANGLE = 4, SB_DRAW_SCALE = 5 };

typedef struct SceneBatchArgs {
  int B;              /* scenes (rows) in the batch, <= SB_MAX_B */
  int N;              /* points per scene */
  int C;              /* channels of the stored cloud: xyz, [rgb], [height] */
  int has_height;     /* the last channel is the height (scaled with the cloud) */
  int augment;        /* student cloud: flip / rotate / scale (training) */
  int ema;            /* also draw ema_point_clouds: an independent, un-augmented sample */
  int vote_rows;      /* rows [0, vote_rows) get vote labels */
  int box_rows;       /* rows [0, box_rows) get box labels */
  int box_aug_rows;   /* of those, rows [0, box_aug_rows) in the student (augmented) frame */
  int NS;             /* size clusters of mean_size */
  unsigned seed, counter;
  int scene[SB_MAX_B];     /* store row of each batch row */
  int scan_idx[SB_MAX_B];  /* written to scan_idx (the index in the row's own scan list) */
  int supervised[SB_MAX_B];/* written to supervised_mask */
  /* the resident store (device pointers) */
  const float *cloud;          /* (P, C) raw cloud, colour normalised, height = z - floor */
  const int *inst;             /* (P,) dense instance id in [0, ninst) */
  const int *sem;              /* (P,) nyu40 semantic id */
  const long long *offset;     /* (S,) first point of each scene */
  const int *count;            /* (S,) points of each scene (>= 1) */
  const int *ninst;            /* (S,) dense instance ids (<= SB_MAX_INST) */
  const double *boxes;         /* (S, SB_MAX_OBJ, SB_BOX_COLS) */
  const int *nbox;             /* (S,) */
  const double *mean_size;     /* (NS, 3) */
  /* explicit draws (parity tests); NULL: draw on the device */
  const int *idx_in;           /* (B, N) student sample, in [0, count) */
  const int *ema_idx_in;       /* (B, N) teacher sample */
  const double *u_in;          /* (B, 4) uniforms in [0,1): flip x, flip y, angle, scale */
  /* scratch */
  int *idx_out;                /* (vote_rows, N) student sample of the vote rows */
  unsigned *table;             /* (vote_rows, SB_MAX_INST, 8) min / max / first position */
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
} SceneBatchArgs;

/* Build one batch: three launches on `stream` (boxes + draws + table clear; sample + augment +
 * per-chunk instance extents; votes).  `args` is a HOST struct of device pointers. */
int scene_batch_build(const SceneBatchArgs *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif
