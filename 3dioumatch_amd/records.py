"""The argument records of the C ABI: every `typedef struct X { ... } X;` of include/*.h, once, as a
ctypes.Structure under the header's own name.

A record is a HOST struct of device pointers that an entry point takes as `const X *`; _lib.py binds
that argument as POINTER(X), so a record of another kind in its place is a ctypes.ArgumentError before
the call.  A pointer field is a c_void_p: assign `tensor.data_ptr()` or None.  This module imports
ctypes only -- neither torch nor the library -- so the host builds of the loss take the same classes.

A new record goes here, under its header, with the header's field names in the header's order;
tests/test_record_abi.py parses the headers and compares names, order, offsets and sizes.
"""
import ctypes

_int, _uint, _ll, _sz = ctypes.c_int, ctypes.c_uint, ctypes.c_longlong, ctypes.c_size_t
_float, _double, _vp = ctypes.c_float, ctypes.c_double, ctypes.c_void_p
_rows = _int * 64  # int[SB_MAX_B]: one entry per batch row


# ---------------------------------------------------------------------------------- include/mlp_hip.h
class MlpOperand(ctypes.Structure):
    _fields_ = ([("mode", _int)] +
                [(n, _vp) for n in ("x", "dz", "scale", "shift", "mean", "invstd", "coef", "argmax")] +
                [(n, _int) for n in ("ns", "groups")] + [("lin_w", _vp)])


# ---------------------------------------------------------------------------------- include/iou3d_hip.h
class EvalMatchArgs(ctypes.Structure):
    _fields_ = ([(n, _int) for n in ("B", "K", "G", "C")] +
                [(n, _vp) for n in ("det", "keep", "det_cls", "gt", "gt_valid", "gt_cls", "ovmax", "jmax")])


class EvalMarkArgs(ctypes.Structure):
    _fields_ = ([("n", _ll), ("num_class", _int), ("num_thresh", _int), ("num_gt", _ll)] +
                [(n, _vp) for n in ("seg", "ovmax", "gt_id", "npos", "thresh", "first", "cum_tp", "rec", "prec",
                                    "ap", "last_rec")])


# ---------------------------------------------------------------------------------- include/lhs_hip.h
class LhsPseudoArgs(ctypes.Structure):
    _fields_ = ([(n, _int) for n in ("S", "K", "NC", "NI", "NH", "NS")] +
                [(n, _float) for n in ("obj_threshold", "cls_threshold", "iou_threshold")] + [("use_nms", _int)] +
                [(n, _vp) for n in ("objectness", "sem_cls", "iou", "heading_scores", "heading_residuals",
                                    "size_scores", "size_residuals", "center", "vote_xyz", "mean_size", "flip_x",
                                    "flip_y", "rot_mat", "scale", "box_center", "box_size", "box_heading",
                                    "box_score", "passed", "negative", "false_xyz", "picked", "label_mask",
                                    "center_label", "false_center_label", "sem_cls_label", "heading_label",
                                    "size_label", "heading_residual_label", "size_residual_label", "iou_label",
                                    "pseudo_gt_ratio")])


class LhsStatsArgs(ctypes.Structure):
    _fields_ = ([(n, _int) for n in ("S", "K", "NC", "NI", "NH", "NS", "labeled", "rows")] +
                [(n, _float) for n in ("obj_threshold", "cls_threshold", "iou_threshold")] +
                [(n, _vp) for n in ("objectness", "sem_cls", "iou", "heading_scores", "heading_residuals",
                                    "size_scores", "size_residuals", "center", "vote_xyz", "mean_size",
                                    "label_mask", "gt_center", "gt_heading_class", "gt_heading_residual",
                                    "gt_size_class", "gt_size_residual", "gt_sem_cls", "gt_box_mask",
                                    "student_objectness", "student_vote_xyz", "flip_x", "flip_y", "rot_mat",
                                    "scale", "iou_labels", "stats", "workspace")])


# ---------------------------------------------------------------------------------- include/loss_hip.h
class VnLossTensor(ctypes.Structure):
    _fields_ = [("p", _vp)] + [(n, _ll) for n in ("sb", "sk", "sc", "sd")]


class VnLossArgs(ctypes.Structure):
    _fields_ = ([(n, _int) for n in ("B", "K", "G", "S", "VF", "N", "NH", "NS", "NC", "NI", "has_jitter",
                                     "consistency")] + [("grad_scale", _float)] +
                [(n, _vp) for n in ("center_label", "box_label_mask", "heading_class_label",
                                    "heading_residual_label", "size_class_label", "size_residual_label",
                                    "sem_cls_label", "vote_label", "vote_label_mask", "seed_inds")] +
                [("seed_inds_stride", _ll), ("mean_size", _vp)] +
                [(n, VnLossTensor) for n in ("agg_xyz", "obj", "center", "h_scores", "h_resn", "s_scores", "s_resn",
                                             "sem", "iou", "iou_jit", "seed_xyz", "vote_xyz", "jit_center",
                                             "jit_size", "jit_heading")] +
                [(n, _vp) for n in ("boxes", "gt_boxes", "iou_lab", "iou_assign", "stats", "objectness_label",
                                    "objectness_mask", "object_assignment", "g_obj", "g_center", "g_h_scores",
                                    "g_h_resn", "g_s_scores", "g_s_resn", "g_sem", "g_iou", "g_iou_jit", "g_vote",
                                    "gt_nearest", "partials")])


# ---------------------------------------------------------------------------------- include/scene_hip.h
class SceneBatchArgs(ctypes.Structure):
    _fields_ = ([(n, _int) for n in ("B", "N", "C", "has_height", "augment", "ema", "vote_rows", "box_rows",
                                     "box_aug_rows", "NS")] + [(n, _uint) for n in ("seed", "counter")] +
                [(n, _rows) for n in ("scene", "scan_idx", "supervised")] +
                [(n, _vp) for n in ("cloud", "inst", "sem", "offset", "count", "ninst", "boxes", "nbox", "mean_size",
                                    "idx_in", "ema_idx_in", "u_in", "idx_out", "table", "point_clouds",
                                    "ema_point_clouds", "vote_label", "vote_label_mask", "center_label",
                                    "heading_class_label", "heading_residual_label", "size_class_label",
                                    "size_residual_label", "sem_cls_label", "box_label_mask", "supervised_mask",
                                    "scan_idx_out", "flip_x_axis", "flip_y_axis", "rot_angle", "rot_mat", "scale")])


# ---------------------------------------------------------------------------------- include/sunrgbd_hip.h
class SunBatchArgs(ctypes.Structure):
    _fields_ = ([(n, _int) for n in ("B", "N", "C", "has_height", "augment", "color_aug", "ema", "vote_rows",
                                     "box_rows", "box_aug_rows", "div256_from", "NS", "num_heading_bin",
                                     "u_point_stride")] + [(n, _uint) for n in ("seed", "counter")] +
                [(n, _rows) for n in ("scene", "scan_idx", "supervised")] +
                [(n, _vp) for n in ("cloud", "votes", "offset", "count", "boxes", "nbox", "mean_size", "idx_in",
                                    "ema_idx_in", "u_in", "u_color_in", "u_point_in", "point_clouds",
                                    "ema_point_clouds", "vote_label", "vote_label_mask", "center_label",
                                    "heading_class_label", "heading_residual_label", "size_class_label",
                                    "size_residual_label", "sem_cls_label", "box_label_mask", "supervised_mask",
                                    "scan_idx_out", "flip_x_axis", "flip_y_axis", "rot_angle", "rot_mat", "scale")])


# ---------------------------------------------------------------------------------- include/scan_hip.h
class ScanPrepareArgs(ctypes.Structure):
    _fields_ = ([("S", _int), ("C", _int)] +
                [(n, _vp) for n in ("cloud", "offset", "count", "floor", "nonfinite")])


class ScanBatchArgs(ctypes.Structure):
    _fields_ = ([(n, _int) for n in ("B", "N", "C", "use_color", "use_height", "dataset")] +
                [(n, _uint) for n in ("seed", "counter")] + [(n, _rows) for n in ("scene", "scan_idx")] +
                [(n, _vp) for n in ("cloud", "offset", "count", "floor", "idx_in", "point_clouds", "scan_idx_out")])


class ScanSemiArgs(ctypes.Structure):
    _fields_ = ([(n, _int) for n in ("B", "N", "C", "use_color", "use_height", "dataset", "row0")] +
                [(n, _uint) for n in ("seed", "counter")] + [(n, _rows) for n in ("scene", "scan_idx")] +
                [(n, _vp) for n in ("cloud", "offset", "count", "floor", "idx_in", "ema_idx_in", "u_in",
                                    "point_clouds", "ema_point_clouds", "flip_x_axis", "flip_y_axis", "rot_angle",
                                    "rot_mat", "scale", "supervised_mask", "scan_idx_out")])


class ScanPackArgs(ctypes.Structure):
    _fields_ = ([(n, _int) for n in ("B", "K", "NC", "scene0")] +
                [(n, _vp) for n in ("keep", "obj_prob", "cls", "score", "center", "size", "heading", "corners",
                                    "count", "proposal", "cls_out", "score_out", "box", "corners_out")])


# ---------------------------------------------------------------------------------- include/scan_tile_hip.h
class ScanBoundsArgs(ctypes.Structure):
    _fields_ = ([(n, _int) for n in ("S", "C", "max_segments")] +
                [(n, _vp) for n in ("cloud", "offset", "count", "partial", "bounds")])


class ScanTileCountArgs(ctypes.Structure):
    _fields_ = ([(n, _int) for n in ("T", "C", "max_segments")] +
                [(n, _vp) for n in ("cloud", "offset", "count", "parent", "window", "counts")])


class ScanTileGatherArgs(ctypes.Structure):
    _fields_ = ([(n, _int) for n in ("T", "C", "max_segments")] + [("rows", _ll)] +
                [(n, _vp) for n in ("cloud", "offset", "count", "parent", "window", "base", "crops")])


class ScanMergeArgs(ctypes.Structure):
    _fields_ = ([(n, _int) for n in ("S", "K", "NC", "cap", "max_tiles")] +
                [(n, _vp) for n in ("first", "tiles", "core", "count_in", "proposal_in", "cls_in", "score_in",
                                    "box_in", "corners_in", "count", "tile", "proposal", "cls", "score", "box",
                                    "corners")])


class ScanSeamArgs(ctypes.Structure):  # "as ScanMergeArgs", then its own tail
    _fields_ = (ScanMergeArgs._fields_ + [(n, _vp) for n in ("iy", "ix", "reach")] + [("thresh", _double)] +
                [(n, _int) for n in ("old_type", "same_class", "dims")] + [("scratch", _vp), ("scratch_bytes", _sz)])


# ---------------------------------------------------------------------------------- include/scan_voxel_hip.h
class ScanVoxelArgs(ctypes.Structure):
    _fields_ = ([(n, _int) for n in ("S", "C", "max_segments", "nearest")] + [("voxel", _double * 3)] +
                [("total_slots", _ll), ("scratch_bytes", _sz)] +
                [(n, _vp) for n in ("cloud", "offset", "count", "slot_offset", "scratch", "slot", "outside")])


class ScanVoxelCountArgs(ctypes.Structure):
    _fields_ = [("mark", ScanVoxelArgs), ("counts", _vp)]


class ScanVoxelGatherArgs(ctypes.Structure):
    _fields_ = [("mark", ScanVoxelArgs), ("rows", _ll)] + [(n, _vp) for n in ("base", "out", "source")]


# ---------------------------------------------------------------------------------- include/point_labels_hip.h
class DetectionsFramesArgs(ctypes.Structure):
    _fields_ = ([(n, _int) for n in ("S", "K", "cap", "NC", "prefer")] + [("min_score", _double)] +
                [(n, _vp) for n in ("count", "cls", "score", "box", "frames", "points", "scratch")] +
                [("scratch_bytes", _sz)])


class PointsLabelArgs(ctypes.Structure):
    _fields_ = ([(n, _int) for n in ("S", "C", "K", "cap", "cull", "max_blocks")] +
                [(n, _vp) for n in ("cloud", "offset", "count", "rows", "frames", "scratch")] +
                [("scratch_bytes", _sz)] + [(n, _vp) for n in ("instance", "semantic", "points")])


# ---------------------------------------------------------------------------------- include/point_index_hip.h
class PointsIndexArgs(ctypes.Structure):
    _fields_ = ([(n, _int) for n in ("S", "cap", "max_segments")] + [("P", _ll)] +
                [(n, _vp) for n in ("key", "offset", "count", "start", "order", "scratch")] + [("scratch_bytes", _sz)])


# ---------------------------------------------------------------------------------- include/mask_eval_hip.h
class MaskOverlapArgs(ctypes.Structure):
    _fields_ = ([(n, _int) for n in ("S", "cap", "G", "max_blocks", "merge", "clear")] +
                [(n, _vp) for n in ("offset", "count", "instance", "truth_instance", "truth_class", "scratch")] +
                [("scratch_bytes", _sz)])


class MaskMatchArgs(ctypes.Structure):
    _fields_ = ([(n, _int) for n in ("S", "cap", "G", "NC", "NS", "min_points", "min_truth_points")] +
                [(n, _vp) for n in ("rows", "cls", "score", "points", "scratch")] + [("scratch_bytes", _sz)] +
                [(n, _vp) for n in ("ovmax", "jmax", "row_score", "key", "klass", "npos")])


# ---------------------------------------------------------------------------------- include/scannet_raw_hip.h
class ScanNetRawArgs(ctypes.Structure):
    _fields_ = ([("S", _int)] + [(n, _ll) for n in ("P", "Q", "T")] +
                [("max_objects", _int), ("max_points", _int), ("seed", _uint)] +
                [(n, _vp) for n in ("raw", "seg", "matrix", "vert_offset", "seg_offset", "seg_label", "seg_object",
                                    "obj_offset", "object_label", "out_offset", "keep", "scan_index", "choice",
                                    "extent", "vert", "ins_label", "sem_label", "bbox", "nbox")])


# ---------------------------------------------------------------------------------- include/sunrgbd_raw_hip.h
class SunRgbdRawArgs(ctypes.Structure):
    _fields_ = ([(n, _int) for n in ("S", "num_point", "elem")] + [("seed", _uint), ("P", _ll)] +
                [(n, _vp) for n in ("raw", "raw_offset", "keep", "scan_index", "choice", "kept", "floor",
                                    "nonfinite", "rows")])
