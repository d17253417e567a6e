/* include/lhs_hip.h -- C ABI of the pseudo-label filter's NMS (semi-supervised step, SURVEY
 * section 8(f) rank 1).  Plain pointers to DEVICE memory, explicit stream, returns hipError_t. */
#ifndef LHS_HIP_H
#define LHS_HIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* replaces the host-side loop of get_pseudo_labels (models/loss_helper_unlabeled.py:447-487):
 * get_3d_box per box (utils/box_util.py:335-358) -> axis-aligned bounds in the camera frame ->
 * lhs_3d_faster_samecls (utils/nms.py:168-214), per scene.  center (scenes,n,3) f32, size
 * (scenes,n,3) f64, heading (scenes,n) f64, score (scenes,n) f32, cls (scenes,n) i64, n <= 64;
 * picked (scenes,n) i32 = 1 for every index the reference's function returns. */
int lhs_nms_samecls(int scenes, int n, const float *center, const double *size,
                    const double *heading, const float *score, const long long *cls, double thresh,
                    int old_type, int *picked, void *stream);

/* replaces the per-scene numpy NMS of the evaluation path (models/ap_helper.py:170-203):
 * nms_3d_faster (same_class = 0, utils/nms.py:77-116) / nms_3d_faster_samecls (same_class = 1,
 * utils/nms.py:118-166) on the axis-aligned camera-frame bounds of get_3d_box
 * (utils/box_util.py:335-358).  Arguments as lhs_nms_samecls; n <= 1024; picked (scenes,n) i32. */
int lhs_nms3d_aabb(int scenes, int n, const float *center, const double *size,
                   const double *heading, const float *score, const long long *cls, double thresh,
                   int old_type, int same_class, int *picked, void *stream);

/* the same NMS on a subset of the boxes, in three or two dimensions: what parse_predictions gets by
 * calling utils/nms.py on boxes[nonempty_box_mask[i,:]==1] (models/ap_helper.py:139-203).
 * valid (scenes,n) i32 or NULL (every box): a box with valid == 0 is neither a winner nor a
 * suppressor and gets picked = 0; a scene with no valid box gives an all-zero row (the reference
 * asserts there).  dims == 3: lhs_nms3d_aabb.  dims == 2: nms_2d_faster (utils/nms.py:52-83) on the
 * camera x / camera z bounds of the same boxes (boxes_2d_with_prob, models/ap_helper.py:143-149);
 * cls is not read and same_class must be 0.  n <= 1024; anything else: hipErrorInvalidValue. */
int lhs_nms_aabb_masked(int scenes, int n, const float *center, const double *size,
                        const double *heading, const float *score, const long long *cls,
                        double thresh, int old_type, int same_class, int dims /* 2 or 3 */,
                        const int *valid /* (scenes,n) i32 or NULL */, int *picked, void *stream);

/* replaces the remove_empty_box loop of parse_predictions (models/ap_helper.py:123-135): B x K
 * calls of extract_pc_in_box3d (sunrgbd/sunrgbd_utils.py:215-224), a Delaunay triangulation of the
 * eight corners and a find_simplex over all points, per box.  count[s][j] = number of points p of
 * scene s with, for d = p - center, c = cos(heading), s = sin(heading):
 *   |c d.x - s d.y| <= l/2,  |s d.x + c d.y| <= w/2,  |d.z| <= h/2
 * (the box frame in float64 rounded to float32, the per-pair arithmetic in float32).  Arguments as
 * lhs_nms3d_aabb; any n.  Non-positive scenes, n or npts: returns 0 without a launch. */
int lhs_box_point_count(int scenes, int n, int npts, int pstride,
                        const float *points,      /* (scenes, npts, pstride) f32, xyz first, depth frame */
                        const float *center,      /* (scenes, n, 3) f32, depth frame */
                        const double *size,       /* (scenes, n, 3) f64  (l, w, h)   */
                        const double *heading,    /* (scenes, n) f64                 */
                        int *count,               /* (scenes, n) i32, written, not accumulated by the caller */
                        void *stream);

/* The rest of the pseudo-label filter around that NMS: get_pseudo_labels and the label transforms
 * of get_unlabeled_loss (models/loss_helper_unlabeled.py:364-445, :489-538, trans_center :24-36,
 * trans_size :39-51) as two launches (select, then -- after lhs_nms_samecls on the select's boxes --
 * finish) instead of ~55 tensor kernels.  All pointers: DEVICE memory, contiguous.  S unlabeled
 * scenes, K teacher proposals each (K <= 1024), n = 64 label slots. */
typedef struct LhsPseudoArgs {
  int S, K, NC, NI, NH, NS;            /* NI: 1 or NC IoU channels */
  float obj_threshold, cls_threshold, iou_threshold;
  int use_nms;                         /* finish: also require picked != 0 */
  /* teacher outputs of the unlabeled scenes */
  const float *objectness;             /* (S,K,2)   */
  const float *sem_cls;                /* (S,K,NC)  */
  const float *iou;                    /* (S,K,NI)  */
  const float *heading_scores;         /* (S,K,NH)  */
  const float *heading_residuals;      /* (S,K,NH)  */
  const float *size_scores;            /* (S,K,NS)  */
  const float *size_residuals;         /* (S,K,NS,3) */
  const float *center;                 /* (S,K,3)   */
  const float *vote_xyz;               /* (S,K,3) aggregated votes */
  const float *mean_size;              /* (NS,3)    */
  /* the student's augmentation of each scene */
  const long long *flip_x, *flip_y;    /* (S)       */
  const float *rot_mat;                /* (S,3,3)   */
  const float *scale;                  /* (S,3)     */
  /* select -> (NMS) -> finish: the 64 best survivors per scene, in score order */
  float *box_center;                   /* (S,64,3) teacher frame              */
  double *box_size;                    /* (S,64,3) float64 decode for the NMS */
  double *box_heading;                 /* (S,64)                              */
  float *box_score;                    /* (S,64) objectness * predicted IoU   */
  int *passed, *negative;              /* (S,64) thresholds passed / objectness < 0.1 */
  float *false_xyz;                    /* (S,64,3) votes of the slots         */
  const int *picked;                   /* (S,64) of lhs_nms_samecls (finish; NULL when !use_nms) */
  /* labels (finish writes label_mask and the transformed centres / size residuals; select the rest) */
  long long *label_mask;               /* (S,64) */
  float *center_label;                 /* (S,64,3) student frame, -1000-based where label_mask = 0 */
  float *false_center_label;           /* (S,64,3) */
  long long *sem_cls_label, *heading_label, *size_label;   /* (S,64) */
  float *heading_residual_label;       /* (S,64) */
  float *size_residual_label;          /* (S,64,3): select the teacher's, finish rescales in place */
  float *iou_label;                    /* (S,64) */
  float *pseudo_gt_ratio;              /* 1: share of slots that passed the thresholds (before NMS) */
} LhsPseudoArgs;
/* scores, threshold masks, the 64 best per scene in score order, their decoded boxes
 * (models/loss_helper_unlabeled.py:364-445); `args`: a HOST struct of DEVICE pointers */
int lhs_pseudo_select(const LhsPseudoArgs *args, void *stream);
/* NMS verdict, -1000 placeholders, labels in the student's frame
 * (models/loss_helper_unlabeled.py:489-538 with trans_center :24-36 and trans_size :39-51) */
int lhs_pseudo_finish(const LhsPseudoArgs *args, void *stream);

/* The `view_stats` logging of the semi-supervised step: the teacher's pseudo labels against the
 * ground truth of the unlabeled scenes (never against the loss).  Order of `stats`: */
enum {
  LHS_STAT_PRED_IOU = 0,        /* unlabeled_pred_iou_value        */
  LHS_STAT_PRED_IOU_OBJ,        /* unlabeled_pred_iou_obj_value    */
  LHS_STAT_IOU_ACC,             /* unlabeled_iou_acc               */
  LHS_STAT_IOU_OBJ_ACC,         /* unlabeled_iou_obj_acc           */
  LHS_STAT_FINAL_IOU,           /* final_iou_avg_value             */
  LHS_STAT_FINAL_IOU_OBJ,       /* final_iou_avg_obj_value         */
  LHS_STAT_FINAL_CLS,           /* final_cls_value                 */
  LHS_STAT_FINAL_CLS_OBJ,       /* final_cls_obj_value             */
  LHS_STAT_COVERAGE_25,         /* final_coverage_0.25_value       */
  LHS_STAT_COVERAGE_50,         /* final_coverage_0.5_value        */
  LHS_STAT_TRUE_OBJ_ACC,        /* true_unlabeled_obj_acc          */
  LHS_STAT_OBJ_ACC,             /* unlabeled_obj_acc (the same value) */
  LHS_STAT_COUNT
};
typedef struct LhsStatsArgs {
  int S, K, NC, NI, NH, NS;            /* as LhsPseudoArgs; 64 GT slots per scene */
  int labeled;                         /* label rows before the unlabeled scenes' */
  int rows;                            /* label rows in all: labeled + S */
  float obj_threshold, cls_threshold, iou_threshold;   /* the filter's (for the slot ranks) */
  /* teacher outputs of the unlabeled scenes, as LhsPseudoArgs */
  const float *objectness, *sem_cls, *iou, *heading_scores, *heading_residuals, *size_scores,
      *size_residuals, *center, *vote_xyz, *mean_size;
  const long long *label_mask;         /* (S,64) of lhs_pseudo_finish: post-NMS slot mask */
  /* ground truth of ALL rows (labeled first), un-augmented frame for the unlabeled rows */
  const float *gt_center;              /* (rows,64,3) */
  const long long *gt_heading_class;   /* (rows,64)   */
  const float *gt_heading_residual;    /* (rows,64)   */
  const long long *gt_size_class;      /* (rows,64)   */
  const float *gt_size_residual;       /* (rows,64,3) */
  const long long *gt_sem_cls;         /* (rows,64)   */
  const float *gt_box_mask;            /* (rows,64)   */
  /* the student's outputs of the unlabeled scenes and their augmentation */
  const float *student_objectness;     /* (S,K,2) */
  const float *student_vote_xyz;       /* (S,K,3) aggregated votes */
  const long long *flip_x, *flip_y;    /* (S)     */
  const float *rot_mat;                /* (S,3,3) */
  const float *scale;                  /* (S,3)   */
  /* outputs and scratch (lhs_pseudo_stats_workspace_bytes(S, K) bytes, no initialisation; it starts
   * with the (S,K) int32 first GT index of every IoU label) */
  float *iou_labels;                   /* (S,K) best same-scene IoU of every teacher proposal */
  float *stats;                        /* (LHS_STAT_COUNT) */
  void *workspace;
} LhsStatsArgs;
/* get_pseudo_labels with view_stats (models/loss_helper_unlabeled.py:392-414, :525-553; IoU labels
 * of models/loss_helper_iou.py:52-112, forward and reverse=True) and the ground-truth objectness of
 * compute_objectness_gt (models/loss_helper_unlabeled.py:82-134, :354-359) in two launches: one
 * over (scene, 16-proposal group) and (scene, 16-GT group) tiles, one workgroup for the sums. */
int lhs_pseudo_stats(const LhsStatsArgs *args, void *stream);
/* bytes of `workspace` for S scenes of K proposals (models/loss_helper_unlabeled.py:392-414) */
size_t lhs_pseudo_stats_workspace_bytes(int S, int K);

#ifdef __cplusplus
}
#endif
#endif /* LHS_HIP_H */
