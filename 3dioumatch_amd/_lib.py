"""ctypes binding of lib3dioumatch_hip.so (the C ABI declared in include/*.h).  PyTorch is used by the callers for device memory and streams only.

There is NO CPU fallback: if the shared library is missing this module raises ImportError,
and every device entry point raises RuntimeError for non-GPU tensors.
"""
import ctypes
import importlib.util
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))


def _load_records():
    """records.py beside this file, ONE module per process under its full name.  The drop-in modules
    load this file by path, and with dropin/ alone on sys.path the package cannot be imported: records.py
    is then loaded by path too, so that every copy of this file, and the package later, binds one class."""
    name = "3dioumatch_amd.records"
    try:
        return importlib.import_module(name)
    except ModuleNotFoundError:
        spec = importlib.util.spec_from_file_location(name, os.path.join(_HERE, "records.py"))
        mod = sys.modules[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod


records = _load_records()
MlpOperand = records.MlpOperand  # (pointnet2._mlp_ext and the tests take it from here)
LIB_PATH = os.path.join(_HERE, "lib3dioumatch_hip%s.so" % os.environ.get("PN2_LIB_SUFFIX", ""))  # (build.py)

_c_int, _c_float, _vp, _sz = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t


def _rec(name):
    """`const <name> *`: a typed pointer to the record of records.py, so that anything but that record
    (or None) in its place -- another record, a raw address, an argument list in another order -- is a
    ctypes.ArgumentError before the call instead of an address the library reads"""
    return ctypes.POINTER(getattr(records, name))


_op = _rec("MlpOperand")  # an operand of the shared-MLP GEMMs

# name -> argtypes (restype is int unless listed in _RESTYPE)
_SIGNATURES = {
    "pn2_furthest_point_sampling": [_c_int, _c_int, _c_int, _vp, _vp, _vp, _vp],
    "pn2_furthest_point_sampling_ws": [_c_int, _c_int, _c_int, _vp, _vp, _vp, _sz, _vp],
    "pn2_fps_workspace_bytes": [_c_int, _c_int, _c_int],
    "pn2_gather_points": [_c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp],
    "pn2_gather_points_grad": [_c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp],
    "pn2_ball_query": [_c_int, _c_int, _c_int, _c_float, _c_int, _vp, _vp, _vp, _vp, _sz, _vp],
    "pn2_ball_query_workspace_bytes": [_c_int, _c_int, _c_int, _c_int],
    "pn2_group_points": [_c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp],
    "pn2_group_points_grad": [_c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp],
    "pn2_three_nn": [_c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp],
    "pn2_three_interpolate": [_c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp],
    "pn2_three_interpolate_affine_supported": [_c_int, _c_int, _c_int],
    "pn2_three_interpolate_affine": [_c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "pn2_three_interpolate_affine_ld": [_c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _c_int, _vp, _vp,
                                        _vp],
    "pn2_three_interpolate_rows_into": [_c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _c_int, _c_int,
                                        _vp, _c_int, _c_int, _vp],
    "pn2_three_interpolate_grad": [_c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp],
    "pn2_three_nn_weights": [ctypes.c_longlong, _vp, _vp, _vp],
    "pn2_multi_copy": [_c_int, _vp, ctypes.c_longlong, _vp],
    "pn2_group_inverse_supported": [_c_int, _c_int, _c_int],
    "pn2_group_inverse_entries": [_c_int, _c_int],
    "pn2_group_inverse_build": [_c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp],
    "pn2_group_points_grad_sorted": [_c_int, _c_int, _c_int, _c_int, _c_int, _vp, _c_int, _c_int, _vp,
                                     _vp, _vp],
    "pn2_three_interpolate_into": [_c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _c_int, _vp],
    "pn2_three_interpolate_grad_from": [_c_int, _c_int, _c_int, _c_int, _vp, _c_int, _vp, _vp, _vp, _vp],
    "pn2_query_and_group": [_c_int, _c_int, _c_int, _c_int, _c_float, _c_int, _c_int, _vp, _vp,
                            _vp, _vp, _vp, _vp, _sz, _vp],
    "pn2_group_concat": [_c_int, _c_int, _c_int, _c_int, _c_float, _c_int, _c_int, _vp, _vp,
                         _vp, _vp, _vp, _vp],
    "pn2_grid_bytes": [_c_int, _c_int],
    "pn2_grid_launch_order": [_c_int, _c_int, _vp, _vp, _vp, _vp],
    "pn2_grid_build": [_c_int, _c_int, _c_float, _vp, _vp, _sz, _vp],
    "pn2_ball_query_prebuilt": [_c_int, _c_int, _c_int, _c_float, _c_int, _vp, _vp, _vp, _vp, _sz, _vp],
    "pn2_query_and_group_prebuilt": [_c_int, _c_int, _c_int, _c_int, _c_float, _c_int, _c_int, _vp,
                                     _vp, _vp, _vp, _vp, _vp, _sz, _vp],
    "pn2_query_and_group_picks": [_c_int, _c_int, _c_int, _c_int, _c_float, _c_int, _c_int, _vp,
                                  _vp, _vp, _vp, _vp, _vp, _sz, _vp],
    "pn2_fps_grid_supported": [_c_int],
    "pn2_furthest_point_sampling_grid": [_c_int, _c_int, _c_int, _vp, _vp, _vp, _sz, _c_float, _vp,
                                         _sz, _vp],
    "pn2_fps_ties_supported": [_c_int],
    "pn2_furthest_point_sampling_ties": [_c_int, _c_int, _c_int, _vp, _vp, _vp, _sz, _c_float, _vp,
                                         _sz, _vp, _vp],
    "pn2_furthest_point_sampling_prefix": [_c_int, _c_int, _c_int, _vp, _vp, _vp, _sz, _vp, _vp],
    "pn2_error_string": [_c_int],
    "mlp_bn_workspace_floats": [_c_int, _c_int, _c_int],
    "mlp_bn_train_stats": [_c_int, _c_int, _c_int, _vp, _vp, _vp, _c_float, _c_float, _vp, _vp, _vp,
                           _vp, _vp, _vp, _vp, _vp, _vp],
    "mlp_bn_eval_coeff": [_c_int, _vp, _vp, _c_float, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "mlp_bn_relu_apply": [_c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp],
    "mlp_bn_relu_pool": [_c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "mlp_bn_relu_backward": [_c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                             _vp, _vp, _vp, _vp, _vp, _vp],
    "mlp_bn_relu_pool_backward": [_c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp,
                                  _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "mlp_bn_relu_backward_stats": [_c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp, _vp,
                                   _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    # the GEMM family: (b, m, k, r), then pointers; _op = a MlpOperand record
    "mlp_gemm_forward": [_c_int] * 4 + [_vp, _vp, _op, _vp, _vp, _vp],
    "mlp_gemm_forward_small": [_c_int] * 4 + [_vp, _c_int, _vp, _op, _vp, _vp, _vp],
    "mlp_gemm_forward_stats_parts": [_c_int, _c_int, _c_int, _c_int, _vp],
    "mlp_bn_finalize_pairs": [_c_int, _c_int, _c_int, _vp, _vp, _vp, _c_float, _c_float, _vp, _vp,
                              _vp, _vp, _vp, _vp, _vp, _vp],
    "mlp_bn_finalize_pairs_scratch_bytes": [_c_int],
    "mlp_gemm_dgrad": [_c_int] * 4 + [_vp, _op, _vp, _vp],
    "mlp_gemm_wgrad": [_c_int] * 4 + [_op, _op, _vp, _vp, _vp],
    "mlp_gemm_wgrad_workspace_floats": [_c_int, _c_int, _c_int, _c_int],
    "mlp_gemm_forward_stats_pool_supported": [_c_int, _c_int, _c_int, _c_int, _c_int],
    "mlp_gemm_forward_stats_pool": [_c_int] * 4 + [_vp, _op, _vp, _vp, _c_int, _vp, _vp, _vp],
    # the pooled last layer's backward from its input's Gram matrix: (b, m, k, r) first
    "mlp_pool_gram_supported": [_c_int] * 5,
    "mlp_pool_gram_parts": [_c_int] * 4,
    "mlp_pool_gram_workspace_floats": [_c_int] * 5,
    "mlp_pool_gram_backward": [_c_int] * 4 + [_vp, _op, _op] + [_vp] * 6,
    "mlp_eval_lin4_supported": [_c_int] * 6,
    "mlp_eval_lin4_pool": [_c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "mlp_eval_stored_supported": [_c_int] * 6,
    "mlp_eval_stored_tiles_per_wave": [_c_int] * 4,
    "mlp_eval_stored_image_bytes": [_c_int],
    "mlp_eval_stored_prepare": [_c_int, _vp, _vp, _vp, _vp],
    "mlp_eval_stored_pool": [_c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "mlp_chain_lin4_parts": [_c_int, _c_int, _c_int, _c_int, _vp],
    "mlp_chain_lin4_image_bytes": [],
    "mlp_chain_lin4_prepare": [_vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "mlp_chain_lin4_stats": [_c_int, _c_int, _c_int, _vp, _vp, _vp, _vp],
    "mlp_chain_lin4_forward": [_c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "mlp_chain_finalize": [_c_int, _c_int, _c_int, _vp, _vp, _vp, _c_float, _c_float, _vp, _vp, _vp, _vp, _vp,
                           _vp, _vp],
    "mlp_bn_pool_from_extrema": [_c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "mlp_wgrad_first4_workspace_bytes": [_c_int, _c_int],
    "mlp_wgrad_first4": [_c_int, _c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "mlp_wgrad_first4_from_gated": [_c_int] + [_vp] * 9,
    "mlp_first4_moments_doubles": [],
    "mlp_first4_moments": [_c_int, _c_int, _vp, _vp, _vp],
    "mlp_first4_bn": [_vp, ctypes.c_double, _vp, _vp, _vp, _c_float, _c_float, _vp, _vp, _vp, _vp, _vp, _vp,
                      _vp],
    "mlp_gemm_backward_fused_supported": [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int],
    "mlp_gemm_backward_fused_workspace_floats": [_c_int, _c_int, _c_int, _c_int],
    "mlp_gemm_backward_fused": [_c_int] * 4 + [_vp, _op, _op] + [_vp] * 5,
    "mlp_gemm_backward_fused_stats_parts": [_c_int, _c_int, _c_int, _c_int],
    "mlp_bn_backward_finalize": [_c_int, _c_int, ctypes.c_double, _c_int, _vp, _vp, _vp, _vp, _vp, _vp,
                                 _vp],
    "mlp_gemm_backward_small_supported": [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int],
    "mlp_weight_image_elems": [_c_int, _c_int],
    "mlp_weight_images_build": [_c_int, _vp, _vp, _vp, _vp, _vp, _vp],
    "mlp_gemm_image_supported": [_c_int, _c_int],
    "mlp_gemm_backward_small": [_c_int] * 4 + [_vp, _vp, _op, _op] + [_vp] * 4,
    "mlp_pregather_supported": [_c_int, _c_int, _c_int, _c_int, _c_int],
    "mlp_pregather_pack": [_c_int, _c_int, _c_int, _c_int, ctypes.c_float, _vp, _vp, _vp, _vp, _vp],
    "mlp_pregather_unpack_grad": [_c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp],
    "mlp_pregather_forward": [_c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp],
    "mlp_pregather_backward": [_c_int] * 5 + [_op, _vp, _vp, _vp],
    "mlp_defer_weight_reductions": [_c_int],
    "mlp_flush_weight_reductions": [],
    "lhs_nms3d_aabb": [_c_int, _c_int, _vp, _vp, _vp, _vp, _vp, ctypes.c_double, _c_int, _c_int, _vp,
                       _vp],
    "lhs_nms_aabb_masked": [_c_int, _c_int, _vp, _vp, _vp, _vp, _vp, ctypes.c_double, _c_int, _c_int,
                            _c_int, _vp, _vp, _vp],
    "lhs_box_point_count": [_c_int] * 4 + [_vp] * 6,
    "votenet_decode_scores": [_c_int] * 5 + [_vp] * 13,
    "votenet_decode_scores_grad": [_c_int] * 5 + [_vp] * 13,
    "lhs_pseudo_select": [_rec("LhsPseudoArgs"), _vp],
    "lhs_pseudo_finish": [_rec("LhsPseudoArgs"), _vp],
    "lhs_pseudo_stats": [_rec("LhsStatsArgs"), _vp],
    "lhs_pseudo_stats_workspace_bytes": [_c_int, _c_int],
    "lhs_nms_samecls": [_c_int, _c_int, _vp, _vp, _vp, _vp, _vp, ctypes.c_double, _c_int, _vp, _vp],
    "iou3d_boxes_overlap_bev": [_c_int, _vp, _c_int, _vp, _vp, _vp],
    "iou3d_boxes_iou_bev": [_c_int, _vp, _c_int, _vp, _vp, _vp],
    "iou3d_boxes_iou3d": [_c_int, _vp, _c_int, _vp, _vp, _vp],
    "iou3d_scene_best_iou3d": [_c_int, _c_int, _vp, _c_int, _vp, _vp, _vp, _vp],
    "votenet_loss_decode": [_rec("VnLossArgs"), _vp],
    "votenet_loss_forward_backward": [_rec("VnLossArgs"), _vp],
    "votenet_loss_scratch_floats": [_rec("VnLossArgs")],
    "votenet_eval_loss_decode": [_rec("VnLossArgs"), _vp],
    "votenet_eval_loss": [_rec("VnLossArgs"), _vp, _vp, _vp],
    "votenet_bbox_jitter": [_c_int, _c_int, _c_int, _c_int] + [_vp] * 15,
    "votenet_gridconv_points": [_c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "votenet_iou_opt_box_step": [_c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp, _c_int, _vp,
                                 _vp, _vp, _vp, _vp, _vp, _c_float, _vp, _vp, _vp, _vp],
    "votenet_vote_tail": [_c_int, _c_int, _c_int] + [_vp] * 7,
    "votenet_vote_tail_grad": [_c_int, _c_int, _c_int] + [_vp] * 8,
    "votenet_iou_score_slices_grad": [_c_int] * 5 + [_vp] * 4,
    "votenet_channel_normalize": [_c_int, _c_int, _c_int, _vp, _vp, _vp, _vp],
    "votenet_channel_normalize_grad": [_c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp],
    "votenet_adam_step": [ctypes.c_longlong, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_double, ctypes.c_double,
                          ctypes.c_double, ctypes.c_double, ctypes.c_double, _vp, _vp, _vp, _vp],
    "votenet_adam_step_guarded": [ctypes.c_longlong, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_double,
                                  ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, _vp,
                                  _vp, _vp, _vp, ctypes.c_double, _vp, _vp, _vp],
    "votenet_adam_guard_partials": [ctypes.c_longlong],
    "votenet_adam_guard_span": [],
    "votenet_guard_state_sync": [ctypes.c_longlong, _vp, _vp, _vp, _vp],
    "votenet_train_meter_add": [_c_int, _vp, _vp, _vp, _vp],
    "iou3d_corners_iou3d": [_c_int, _vp, _c_int, _vp, _vp, _vp],
    "iou3d_corners_best_match": [_c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "iou3d_eval_match": [_rec("EvalMatchArgs"), _vp],
    "iou3d_eval_mark": [_rec("EvalMarkArgs"), _vp],
    "iou3d_nms_mask": [_vp, _vp, _c_int, _c_float, _vp],
    "iou3d_nms_normal_mask": [_vp, _vp, _c_int, _c_float, _vp],
    "iou3d_nms": [_vp, _c_int, _c_float, _c_int, _vp, _vp, _vp, _vp],
    "iou3d_boxes_iou_bev_cpu": [_c_int, _vp, _c_int, _vp, _vp],
}
_RESTYPE = {"pn2_ball_query_workspace_bytes": _sz, "lhs_pseudo_stats_workspace_bytes": _sz, "pn2_grid_bytes": _sz, "pn2_fps_workspace_bytes": _sz, "mlp_bn_workspace_floats": _sz, "mlp_gemm_wgrad_workspace_floats": _sz, "mlp_wgrad_first4_workspace_bytes": _sz, "mlp_gemm_backward_fused_workspace_floats": _sz, "mlp_bn_finalize_pairs_scratch_bytes": _sz, "mlp_chain_lin4_image_bytes": _sz, "mlp_eval_stored_image_bytes": _sz, "mlp_weight_image_elems": _sz, "mlp_pool_gram_workspace_floats": _sz, "scene_detections_merge_nms_scratch_bytes": _sz, "scene_scan_voxel_slots": ctypes.c_longlong, "scene_points_label_scratch_bytes": _sz, "scene_points_index_scratch_bytes": _sz, "scene_mask_scratch_bytes": _sz, "pn2_error_string": ctypes.c_char_p}

EXPORTS = tuple(_SIGNATURES)

# the batch builders (include/scene_hip.h: ScanNet, include/sunrgbd_hip.h: SUN RGB-D): the data
# loaders' entry points, bound with the rest but outside EXPORTS, which is the drop-in surface of the
# reference's kernels
_LOADER_SIGNATURES = {
    "scene_batch_build": [_rec("SceneBatchArgs"), _vp],
    "scene_sunrgbd_batch_build": [_rec("SunBatchArgs"), _vp],
    "scene_sunrgbd_votes": [_vp, _c_int, _vp, _vp, _vp, _vp, _c_int, _vp, _vp],
    # the label-free scan path (include/scan_hip.h)
    "scene_scan_prepare": [_rec("ScanPrepareArgs"), _vp],
    "scene_scan_batch_build": [_rec("ScanBatchArgs"), _vp],
    "scene_scan_semi_build": [_rec("ScanSemiArgs"), _vp],
    "scene_detections_pack": [_rec("ScanPackArgs"), _vp],
    # scans larger than a room: device tiling and merged detections (include/scan_tile_hip.h)
    "scene_scan_bounds": [_rec("ScanBoundsArgs"), _vp],
    "scene_scan_tile_count": [_rec("ScanTileCountArgs"), _vp],
    "scene_scan_tile_gather": [_rec("ScanTileGatherArgs"), _vp],
    "scene_detections_merge": [_rec("ScanMergeArgs"), _vp],
    "scene_detections_merge_nms": [_rec("ScanSeamArgs"), _vp],
    "scene_detections_merge_nms_scratch_bytes": [_c_int, _c_int, _c_int, _c_int],
    # voxel-grid downsample of scan stores (include/scan_voxel_hip.h)
    "scene_scan_voxel_slots": [_c_int],
    "scene_scan_voxel_mark": [_rec("ScanVoxelArgs"), _vp],
    "scene_scan_voxel_count": [_rec("ScanVoxelCountArgs"), _vp],
    "scene_scan_voxel_gather": [_rec("ScanVoxelGatherArgs"), _vp],
    # per-point instance labels from packed detections (include/point_labels_hip.h)
    "scene_points_label_scratch_bytes": [_c_int, _c_int],
    "scene_detections_frames": [_rec("DetectionsFramesArgs"), _vp],
    "scene_points_label": [_rec("PointsLabelArgs"), _vp],
    # per-detection point lists: a stable multi-split of the label plane (include/point_index_hip.h)
    "scene_points_index_scratch_bytes": [_c_int, _c_int, _c_int, ctypes.c_longlong],
    "scene_points_index": [_rec("PointsIndexArgs"), _vp],
    # mask matching of point labels against ground-truth instances (include/mask_eval_hip.h)
    "scene_mask_scratch_bytes": [_c_int, _c_int, _c_int],
    "scene_mask_overlap": [_rec("MaskOverlapArgs"), _vp],
    "scene_mask_match": [_rec("MaskMatchArgs"), _vp],
    # raw ScanNet scans -> the preprocessed layout (include/scannet_raw_hip.h)
    "scannet_raw_export": [_rec("ScanNetRawArgs"), _vp],
    # raw SUN RGB-D depth clouds -> kept rows, floors, store rows (include/sunrgbd_raw_hip.h)
    "scene_sunrgbd_raw_export": [_rec("SunRgbdRawArgs"), _vp],
}


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "3dioumatch_amd: %s is missing -- build it with `python 3dioumatch_amd/build.py` "
            "(hipcc, gfx950). There is no CPU fallback." % LIB_PATH)
    # PyTorch-ROCm ships its own HIP runtime; load it FIRST so that this library binds to the
    # runtime that owns the process's device context (dlopen-ing the library before `import torch`
    # pulled in /opt/rocm's copy: two runtimes in one process, "no ROCm-capable device" at the
    # first launch -- seen with __graft_entry__.build() followed by smoke() in one interpreter)
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    for name, argtypes in list(_SIGNATURES.items()) + list(_LOADER_SIGNATURES.items()):
        fn = getattr(lib, name)  # AttributeError here == ABI mismatch, fail loudly
        fn.argtypes = argtypes
        fn.restype = _RESTYPE.get(name, _c_int)
    return lib


lib = _load()


def check(code, what):
    """Turn a non-zero hipError_t return into a Python exception (never exit())."""
    if code != 0:
        msg = lib.pn2_error_string(int(code))
        raise RuntimeError("%s failed: HIP error %d (%s)" %
                           (what, code, msg.decode() if msg else "?"))


def current_stream_ptr(device):
    import torch
    return torch.cuda.current_stream(device).cuda_stream


def run(entry, record, device, *more, stream=None):
    """Call the record entry point `entry(&record, *more, stream)` with `device` current, on the raw
    `stream` (None: the device's current stream): the one place that launches with a record."""
    import torch
    with torch.cuda.device(device):
        check(getattr(lib, entry)(ctypes.byref(record), *more,
                                  current_stream_ptr(device) if stream is None else stream), entry)
