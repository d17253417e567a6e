/* scan_hip.h -- C ABI of the label-free scan path (csrc/scan_batch.hip): the resident store of raw
 * scans (votenet/scan_data.py:ScanStore), its batches (ScanLoader) and the packed detections of
 * votenet/detect.py.
 *
 * What the reference does per __getitem__ on the host for a scan without labels -- the floor height
 * np.percentile(z, 0.99), the colour normalisation, the height channel and the point sample -- and
 * what ap_helper.parse_predictions lists on the host per batch is done here by three launches.  The
 * draws are the counter-based hash of scene_hip.h (csrc/scene_common.h), so a ScanLoader batch is
 * the eval batch of the labeled loaders for the same (seed, counter, row).  Every argument record
 * is a HOST struct of device pointers handed to the kernels by value; nothing is copied host ->
 * device per batch.
 */
#ifndef SCAN_HIP_H
#define SCAN_HIP_H

#include "scene_hip.h" /* SB_MAX_B, SB_DRAW_STUDENT */

#ifdef __cplusplus
extern "C" {
#endif

#define SCAN_MAX_K 1024 /* proposals per scene (the NMS kernels' own limit) */

enum { SCAN_DATASET_SCANNET = 0, SCAN_DATASET_SUNRGBD = 1 };

typedef struct ScanPrepareArgs {
  int S;                   /* scans in the store */
  int C;                   /* columns of the raw rows: 3 (xyz) or 6 (xyz rgb) */
  const float *cloud;      /* (P, C) raw rows of every scan */
  const long long *offset; /* (S,) first row of each scan */
  const int *count;        /* (S,) rows of each scan, 1 <= count < 2^30 */
  float *floor;            /* (S,) out: np.percentile(z, 0.99) in float32 */
  int *nonfinite;          /* (S,) out: NaN / Inf values among the scan's count * C numbers */
} ScanPrepareArgs;

/* Per scan, one workgroup: the floor height every __getitem__ of the reference recomputes
 * (scannet/scannet_detection_dataset.py:129, sunrgbd/sunrgbd_detection_dataset.py:149:
 * floor_height = np.percentile(point_cloud[:,2],0.99)) by an exact radix select of the two order
 * statistics numpy interpolates and numpy's own float32 lerp, un-contracted; and the count of
 * non-finite values the store's constructor refuses. */
int scene_scan_prepare(const ScanPrepareArgs *args, void *stream);

typedef struct ScanBatchArgs {
  int B;              /* scans (rows) in the batch, <= SB_MAX_B */
  int N;              /* points per row */
  int C;              /* columns of the raw rows: 3 or 6 */
  int use_color;      /* output channels 3..5: normalised rgb (needs C == 6) */
  int use_height;     /* last output channel: z - floor */
  int dataset;        /* SCAN_DATASET_*: which colour normalisation */
  unsigned seed, counter;
  int scene[SB_MAX_B];    /* store row of each batch row */
  int scan_idx[SB_MAX_B]; /* written to scan_idx_out */
  const float *cloud;      /* (P, C) */
  const long long *offset; /* (S,) */
  const int *count;        /* (S,) */
  const float *floor;      /* (S,) scene_scan_prepare's */
  const int *idx_in;       /* (B, N) explicit sample in [0, count) (parity tests); NULL: drawn */
  float *point_clouds;     /* (B, N, 3 + 3 use_color + use_height) out */
  long long *scan_idx_out; /* (B,) out */
} ScanBatchArgs;

/* One launch: the eval rows of the two detection datasets for scans without labels
 * (scannet/scannet_detection_dataset.py:85-223, sunrgbd/sunrgbd_detection_dataset.py:119-246 with
 * augment=False): pc_util.random_sampling (utils/pc_util.py:35-43; draw SB_DRAW_STUDENT of the
 * row), the colour normalisation rounded once from double ((rgb - MEAN_COLOR_RGB) / 256 for
 * ScanNet, rgb - 0.5 for SUN RGB-D) and height = z - floor in float32. */
int scene_scan_batch_build(const ScanBatchArgs *args, void *stream);

typedef struct ScanSemiArgs {
  int B;              /* unlabeled rows built here, 1..SB_MAX_B */
  int N;              /* points per row */
  int C;              /* columns of the raw rows: 3 or 6 */
  int use_color;      /* output channels 3..5: normalised rgb (needs C == 6) */
  int use_height;     /* last output channel: z - floor, scaled with the student's cloud */
  int dataset;        /* SCAN_DATASET_*: colour normalisation and augmentation */
  int row0;           /* labeled rows in front: row r here is batch row row0 + r, which keys its draws */
  unsigned seed, counter;
  int scene[SB_MAX_B];    /* store row of each row */
  int scan_idx[SB_MAX_B]; /* written to scan_idx_out */
  const float *cloud;      /* (P, C) */
  const long long *offset; /* (S,) */
  const int *count;        /* (S,) */
  const float *floor;      /* (S,) scene_scan_prepare's */
  /* explicit draws (parity tests), indexed by r; NULL: drawn on the device */
  const int *idx_in;       /* (B, N) student sample in [0, count) */
  const int *ema_idx_in;   /* (B, N) teacher sample */
  const double *u_in;      /* (B, 4) ScanNet: flip x, flip y, angle, scale; (B, 3) SUN RGB-D: flip, angle, scale */
  /* outputs: row r of each is batch row row0 + r (the trailing rows of the batch's tensors) */
  float *point_clouds;     /* (B, N, 3 + 3 use_color + use_height) student sample, augmented */
  float *ema_point_clouds; /* (B, N, same) teacher sample, not augmented */
  long long *flip_x_axis, *flip_y_axis; /* (B,) */
  float *rot_angle;        /* (B,) */
  float *rot_mat;          /* (B, 3, 3) */
  float *scale;            /* (B, 1, 3) */
  long long *supervised_mask; /* (B,) out: 0 */
  long long *scan_idx_out; /* (B,) out */
} ScanSemiArgs;

/* One launch, (chunks of 2048 slots) x rows x (student, teacher): the UNLABELED rows of a
 * semi-supervised batch (scannet/scannet_ssl_dataset.py:224-320, sunrgbd/sunrgbd_ssl_dataset.py:
 * 221-312) from raw clouds.  Each slot gathers its raw row (draws SB_DRAW_STUDENT / SB_DRAW_EMA of
 * batch row row0 + r), normalises colour as scene_scan_batch_build does -- SUN RGB-D divides by 256
 * once more in float32, as its unlabeled dataset does -- and takes height = z - floor; the student
 * sample then goes through the dataset's augmentation by the very device functions
 * scene_batch_build / scene_sunrgbd_batch_build call (csrc/scene_common.h: float64 per stage,
 * rounded to float32 after each), so the rows are bit-equal to the unlabeled rows those builders
 * give for the same scans as float32 files.  One thread per row writes the row's header with the
 * function their box kernels write it with.
 * hipErrorInvalidValue, without a launch: NULL args, B outside 1..SB_MAX_B, row0 < 0 or row0 + B >
 * SB_MAX_B, N < 1, C not 3 or 6, use_color with C == 3, an unknown dataset, a NULL store or output
 * pointer. */
int scene_scan_semi_build(const ScanSemiArgs *args, void *stream);

typedef struct ScanPackArgs {
  int B;                    /* scenes of the batch */
  int K;                    /* proposals per scene, <= SCAN_MAX_K; also the rows per scene (cap) */
  int NC;                   /* > 0: per-class scores (B, K, NC); 0: one score per proposal */
  int scene0;               /* arena row of the batch's first scene */
  /* the batch (device pointers) */
  const unsigned char *keep; /* (B, K) bool: the detections */
  const float *obj_prob;     /* (B, K) the ordering key */
  const long long *cls;      /* (B, K) arg-max class */
  const float *score;        /* (B, K) or (B, K, NC) */
  const float *center;       /* (B, K, 3) */
  const double *size;        /* (B, K, 3) decoded l, w, h */
  const double *heading;     /* (B, K) decoded heading */
  const float *corners;      /* (B, K, 8, 3) upright camera frame */
  /* the arena's planes, each indexed by arena row (scene0 + scene) */
  int *count;                /* (S,) */
  int *proposal;             /* (S, K) */
  int *cls_out;              /* (S, K) */
  float *score_out;          /* (S, K) or (S, K, NC) */
  float *box;                /* (S, K, 7) centre, size, heading (network frame) */
  float *corners_out;        /* (S, K, 8, 3) */
} ScanPackArgs;

/* One launch, one workgroup per scene: what ap_helper.parse_predictions lists on the host per
 * batch (models/ap_helper.py:205-219: the proposals with pred_mask == 1 and obj_prob >
 * conf_thresh) written compacted into the run's arena, ordered by objectness probability
 * descending, ties by proposal index ascending (a rank by counting, csrc/pseudo_rank.h); rows past
 * `count` are zero. */
int scene_detections_pack(const ScanPackArgs *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif
