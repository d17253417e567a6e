"""Device-side NMS of the pseudo-label filter (binding of include/lhs_hip.h).

The reference copies the 64 best teacher predictions of every unlabeled scene to the host, builds
their 3-D boxes one by one in numpy and runs utils/nms.py:lhs_3d_faster_samecls
(models/loss_helper_unlabeled.py:447-487); here the same computation is one kernel launch with no
host round trip, so the semi-supervised step stays capturable in a HIP graph.
"""
import torch

from .. import _lib as _L
from .. import records

_lib = _L.lib


def lhs_nms_samecls_gpu(center, size, heading, score, cls, thresh, old_type=False):
    """center (S,n,3) f32, size (S,n,3) f64, heading (S,n) f64, score (S,n) f32, cls (S,n) i64 ->
    picked (S,n) bool: True for the boxes lhs_3d_faster_samecls keeps (n <= 64)."""
    for t, dt, name in ((center, torch.float32, "center"), (size, torch.float64, "size"),
                        (heading, torch.float64, "heading"), (score, torch.float32, "score"),
                        (cls, torch.int64, "cls")):
        if not t.is_cuda or t.dtype != dt:
            raise RuntimeError("%s must be a %s GPU tensor" % (name, dt))
    s, n = score.shape
    if n > 64:
        raise RuntimeError("lhs_nms_samecls: at most 64 boxes per scene (MAX_NUM_OBJ)")
    picked = torch.zeros((s, n), dtype=torch.int32, device=score.device)
    # contiguous copies (if any) stay bound to locals until after the launch: a temporary's block
    # could be handed to the next allocation on this stream before the kernel has read it
    center, size, heading, score, cls = (t.contiguous() for t in (center, size, heading, score, cls))
    with torch.cuda.device(score.device):
        _L.check(_lib.lhs_nms_samecls(s, n, center.data_ptr(), size.data_ptr(), heading.data_ptr(),
                                      score.data_ptr(), cls.data_ptr(),
                                      float(thresh), 1 if old_type else 0, picked.data_ptr(),
                                      _L.current_stream_ptr(score.device)), "lhs_nms_samecls")
    return picked.bool()


def nms3d_aabb_gpu(center, size, heading, score, cls, thresh, old_type=False, same_class=True):
    """The evaluation path's per-scene NMS (utils/nms.py nms_3d_faster / nms_3d_faster_samecls on
    the camera-frame bounds of every proposal) -> picked (S,n) bool, n <= 1024 (one workgroup per scene: 256 lanes up to 256 boxes,
    1024 lanes beyond)."""
    for t, dt, name in ((center, torch.float32, "center"), (size, torch.float64, "size"),
                        (heading, torch.float64, "heading"), (score, torch.float32, "score"),
                        (cls, torch.int64, "cls")):
        if not t.is_cuda or t.dtype != dt:
            raise RuntimeError("%s must be a %s GPU tensor" % (name, dt))
    s, n = score.shape
    if n > 1024:
        raise RuntimeError("nms3d_aabb: at most 1024 boxes per scene")
    picked = torch.zeros((s, n), dtype=torch.int32, device=score.device)
    center, size, heading, score, cls = (t.contiguous() for t in (center, size, heading, score, cls))
    with torch.cuda.device(score.device):
        _L.check(_lib.lhs_nms3d_aabb(s, n, center.data_ptr(), size.data_ptr(), heading.data_ptr(),
                                     score.data_ptr(), cls.data_ptr(),
                                     float(thresh), 1 if old_type else 0, 1 if same_class else 0,
                                     picked.data_ptr(), _L.current_stream_ptr(score.device)),
                 "lhs_nms3d_aabb")
    return picked.bool()


def nms_aabb_masked_gpu(center, size, heading, score, cls, thresh, old_type=False, same_class=True,
                        dims=3, valid=None):
    """nms3d_aabb_gpu on the boxes with valid != 0 only (valid (S,n) i32 or None for all; the
    reference's boxes[nonempty_box_mask[i,:]==1], models/ap_helper.py:139-203): a masked box is
    neither winner nor suppressor and is not picked, a scene without a valid box gives an all-False
    row.  dims=2: utils/nms.py nms_2d_faster on the camera x / z bounds; `cls` may be None and
    same_class must be False."""
    if dims not in (2, 3):
        raise RuntimeError("nms_aabb_masked: dims must be 2 or 3")
    if dims == 2 and same_class:
        raise RuntimeError("nms_aabb_masked: the 2-D NMS has no same-class form")
    if dims == 3 and cls is None:
        raise RuntimeError("nms_aabb_masked: cls is required for dims = 3")
    ins = [(center, torch.float32, "center"), (size, torch.float64, "size"),
           (heading, torch.float64, "heading"), (score, torch.float32, "score")]
    if cls is not None:
        ins.append((cls, torch.int64, "cls"))
    if valid is not None:
        ins.append((valid, torch.int32, "valid"))
    for t, dt, name in ins:
        if not t.is_cuda or t.dtype != dt:
            raise RuntimeError("%s must be a %s GPU tensor" % (name, dt))
    s, n = score.shape
    if n > 1024:
        raise RuntimeError("nms_aabb_masked: at most 1024 boxes per scene")
    if valid is not None and tuple(valid.shape) != (s, n):
        raise RuntimeError("nms_aabb_masked: valid must be (%d, %d)" % (s, n))
    picked = torch.zeros((s, n), dtype=torch.int32, device=score.device)
    center, size, heading, score = (t.contiguous() for t in (center, size, heading, score))
    cls = cls.contiguous() if cls is not None else None
    valid = valid.contiguous() if valid is not None else None
    with torch.cuda.device(score.device):
        _L.check(_lib.lhs_nms_aabb_masked(s, n, center.data_ptr(), size.data_ptr(), heading.data_ptr(),
                                          score.data_ptr(), cls.data_ptr() if cls is not None else None,
                                          float(thresh), 1 if old_type else 0, 1 if same_class else 0,
                                          dims, valid.data_ptr() if valid is not None else None,
                                          picked.data_ptr(), _L.current_stream_ptr(score.device)),
                 "lhs_nms_aabb_masked")
    return picked.bool()


BOX_POINT_CHUNK = 512  # points one workgroup of the count kernel stages (csrc/box_points.hip)


def box_point_count_gpu(points, center, size, heading, out=None):
    """points (S,N,3+C) f32 with xyz first, center (S,n,3) f32, size (S,n,3) f64 (l,w,h), heading
    (S,n) f64, all in the depth frame -> count (S,n) int32: the points inside each oriented box,
    len(extract_pc_in_box3d(...)[0]) of models/ap_helper.py:123-135 by the closed-form test of
    include/lhs_hip.h.  `points` is read in place through its row stride (no xyz slice copy).
    `out`: an (S,n) int32 tensor to overwrite (the entry point zero-fills it itself)."""
    for t, dt, name in ((points, torch.float32, "points"), (center, torch.float32, "center"),
                        (size, torch.float64, "size"), (heading, torch.float64, "heading")):
        if not t.is_cuda or t.dtype != dt:
            raise RuntimeError("%s must be a %s GPU tensor" % (name, dt))
    s, n = heading.shape
    if points.dim() != 3 or points.shape[0] != s or points.shape[2] < 3:
        raise RuntimeError("box_point_count: points must be (%d, N, >= 3)" % s)
    if tuple(center.shape) != (s, n, 3) or tuple(size.shape) != (s, n, 3):
        raise RuntimeError("box_point_count: center and size must be (%d, %d, 3)" % (s, n))
    npts, pstride = points.shape[1], points.shape[2]
    if out is None:
        out = torch.empty((s, n), dtype=torch.int32, device=heading.device)
    elif not out.is_cuda or out.dtype != torch.int32 or tuple(out.shape) != (s, n) or not out.is_contiguous():
        raise RuntimeError("box_point_count: out must be a contiguous (%d, %d) int32 GPU tensor" % (s, n))
    count = out
    if npts == 0 or s == 0 or n == 0:
        return count.zero_()     # nothing to launch
    points, center, size, heading = (t.contiguous() for t in (points, center, size, heading))
    with torch.cuda.device(heading.device):
        _L.check(_lib.lhs_box_point_count(s, n, npts, pstride, points.data_ptr(), center.data_ptr(),
                                          size.data_ptr(), heading.data_ptr(), count.data_ptr(),
                                          _L.current_stream_ptr(heading.device)), "lhs_box_point_count")
    return count


def pseudo_labels_supported(pred_center, scale, f32=(), i64=(), sem_cls=None, iou_scores=None):
    """The two-launch form covers GPU tensors, 64 <= K <= 1024 proposals, a per-axis scale (S,1,3),
    float32 network outputs (`f32`), int64 flip flags (`i64`) on the same device and one IoU score
    per proposal or per class.  Anything else -- bool flags, an autocast teacher -- is the tensor
    implementation's (get_pseudo_labels), not an error."""
    dev = pred_center.device
    if not (pred_center.is_cuda and 64 <= pred_center.shape[1] <= 1024 and
            tuple(scale.shape) == (pred_center.shape[0], 1, 3)):
        return False
    if any(t.dtype != torch.float32 or t.device != dev for t in (pred_center, scale, *f32)):
        return False
    if any(t.dtype != torch.int64 or t.device != dev for t in i64):
        return False
    if sem_cls is not None and iou_scores is not None and iou_scores.shape[2] not in (1, sem_cls.shape[2]):
        return False
    return True


def pseudo_labels_gpu(objectness, sem_cls, iou_scores, heading_scores, heading_residuals, size_scores,
                      size_residuals, center, vote_xyz, mean_size, flip_x, flip_y, rot_mat, scale,
                      obj_threshold, cls_threshold, iou_threshold, nms=None):
    """get_pseudo_labels + trans_center / trans_size of losses_unlabeled.py as two launches around
    the NMS kernel (include/lhs_hip.h lhs_pseudo_select / lhs_pseudo_finish).  `nms`: None, or
    (iou threshold, old_type) for lhs_nms_samecls on the selected boxes.  Returns a dict with
    label_mask, center_label, false_center_label, sem_cls_label, heading_label,
    heading_residual_label, size_label, size_residual_label, iou_label, pseudo_gt_ratio."""
    dev = center.device
    s, k = center.shape[:2]
    f32 = dict(dtype=torch.float32, device=dev)
    i64 = dict(dtype=torch.int64, device=dev)
    keep = []

    def inp(t, dt):
        if t.dtype != dt or t.device != dev:
            raise RuntimeError("pseudo_labels_gpu: expected %s tensors on %s" % (dt, dev))
        t = t.detach().contiguous()
        keep.append(t)
        return t.data_ptr()
    a = records.LhsPseudoArgs()
    a.S, a.K = s, k
    a.NC, a.NI, a.NH, a.NS = sem_cls.shape[2], iou_scores.shape[2], heading_scores.shape[2], size_scores.shape[2]
    a.obj_threshold, a.cls_threshold, a.iou_threshold = float(obj_threshold), float(cls_threshold), float(iou_threshold)
    a.use_nms = 1 if nms is not None else 0
    for name, t in (("objectness", objectness), ("sem_cls", sem_cls), ("iou", iou_scores),
                    ("heading_scores", heading_scores), ("heading_residuals", heading_residuals),
                    ("size_scores", size_scores), ("size_residuals", size_residuals), ("center", center),
                    ("vote_xyz", vote_xyz), ("mean_size", mean_size), ("rot_mat", rot_mat), ("scale", scale)):
        setattr(a, name, inp(t, torch.float32))
    a.flip_x, a.flip_y = inp(flip_x, torch.int64), inp(flip_y, torch.int64)
    n = 64
    out = {"label_mask": torch.empty((s, n), **i64), "center_label": torch.empty((s, n, 3), **f32),
           "false_center_label": torch.empty((s, n, 3), **f32), "sem_cls_label": torch.empty((s, n), **i64),
           "heading_label": torch.empty((s, n), **i64), "size_label": torch.empty((s, n), **i64),
           "heading_residual_label": torch.empty((s, n), **f32),
           "size_residual_label": torch.empty((s, n, 3), **f32), "iou_label": torch.empty((s, n), **f32),
           "pseudo_gt_ratio": torch.empty((), **f32)}
    box_center = torch.empty((s, n, 3), **f32)
    box_size = torch.empty((s, n, 3), dtype=torch.float64, device=dev)
    box_heading = torch.empty((s, n), dtype=torch.float64, device=dev)
    box_score = torch.empty((s, n), **f32)
    flags = torch.empty((2, s, n), dtype=torch.int32, device=dev)
    false_xyz = torch.empty((s, n, 3), **f32)
    a.box_center, a.box_size, a.box_heading = box_center.data_ptr(), box_size.data_ptr(), box_heading.data_ptr()
    a.box_score, a.passed, a.negative = box_score.data_ptr(), flags[0].data_ptr(), flags[1].data_ptr()
    a.false_xyz = false_xyz.data_ptr()
    for name, t in out.items():
        setattr(a, name, t.data_ptr())
    _L.run("lhs_pseudo_select", a, dev)
    if nms is not None:
        picked = torch.zeros((s, n), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _L.check(_lib.lhs_nms_samecls(s, n, box_center.data_ptr(), box_size.data_ptr(), box_heading.data_ptr(),
                                          box_score.data_ptr(), out["sem_cls_label"].data_ptr(), float(nms[0]),
                                          1 if nms[1] else 0, picked.data_ptr(), _L.current_stream_ptr(dev)),
                     "lhs_nms_samecls")
        a.picked = picked.data_ptr()
    _L.run("lhs_pseudo_finish", a, dev)
    return out


# order of the kernel's `stats` output (include/lhs_hip.h LHS_STAT_*)
STAT_KEYS = ("unlabeled_pred_iou_value", "unlabeled_pred_iou_obj_value", "unlabeled_iou_acc",
             "unlabeled_iou_obj_acc", "final_iou_avg_value", "final_iou_avg_obj_value", "final_cls_value",
             "final_cls_obj_value", "final_coverage_0.25_value", "final_coverage_0.5_value",
             "true_unlabeled_obj_acc", "unlabeled_obj_acc")


def pseudo_label_stats_gpu(objectness, sem_cls, iou_scores, heading_scores, heading_residuals, size_scores,
                           size_residuals, center, vote_xyz, mean_size, label_mask, gt, labeled,
                           student_objectness, student_vote_xyz, flip_x, flip_y, rot_mat, scale,
                           obj_threshold, cls_threshold, iou_threshold, assignment=False):
    """The view_stats numbers of get_pseudo_labels / compute_objectness_gt in two launches
    (include/lhs_hip.h lhs_pseudo_stats), to run after pseudo_labels_gpu: teacher outputs and
    augmentation as pseudo_labels_gpu takes them, `label_mask` (S,64) its output, `gt` the seven
    box-label tensors (data.BOX_LABEL_KEYS) of ALL rows -- `labeled` rows first, then the S unlabeled scenes in the
    teacher's frame -- and the student's objectness scores / aggregated votes of the unlabeled scenes.
    Returns {'unlabeled_iou_labels': (S,K) f32, one 0-dim f32 tensor per STAT_KEYS entry} (with
    `assignment`, also 'unlabeled_iou_assignment': the (S,K) first GT index of each IoU label);
    nothing leaves the device and no input is written."""
    dev = center.device
    s, k = center.shape[:2]
    keep = []

    def inp(t, dt, shape=None):
        if t.dtype != dt or t.device != dev:
            raise RuntimeError("pseudo_label_stats_gpu: expected %s tensors on %s" % (dt, dev))
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise RuntimeError("pseudo_label_stats_gpu: shape %s, expected %s" % (tuple(t.shape), shape))
        t = t.detach().contiguous()
        keep.append(t)
        return t.data_ptr()
    rows = labeled + s
    a = records.LhsStatsArgs()
    a.S, a.K, a.labeled, a.rows = s, k, labeled, rows
    a.NC, a.NI, a.NH, a.NS = sem_cls.shape[2], iou_scores.shape[2], heading_scores.shape[2], size_scores.shape[2]
    a.obj_threshold, a.cls_threshold, a.iou_threshold = float(obj_threshold), float(cls_threshold), float(iou_threshold)
    f32, i64 = torch.float32, torch.int64
    for name, t, shape in (("objectness", objectness, (s, k, 2)), ("sem_cls", sem_cls, None), ("iou", iou_scores, None),
                           ("heading_scores", heading_scores, None), ("heading_residuals", heading_residuals, None),
                           ("size_scores", size_scores, None), ("size_residuals", size_residuals, None),
                           ("center", center, (s, k, 3)), ("vote_xyz", vote_xyz, (s, k, 3)),
                           ("mean_size", mean_size, (a.NS, 3)), ("student_objectness", student_objectness, (s, k, 2)),
                           ("student_vote_xyz", student_vote_xyz, (s, k, 3)), ("rot_mat", rot_mat, (s, 3, 3)),
                           ("scale", scale, (s, 1, 3))):
        setattr(a, name, inp(t, f32, shape))
    a.flip_x, a.flip_y = inp(flip_x, i64, (s,)), inp(flip_y, i64, (s,))
    a.label_mask = inp(label_mask, i64, (s, 64))
    for name, key, dt, tail in (("gt_center", "center_label", f32, (3,)), ("gt_heading_class", "heading_class_label", i64, ()),
                                ("gt_heading_residual", "heading_residual_label", f32, ()),
                                ("gt_size_class", "size_class_label", i64, ()),
                                ("gt_size_residual", "size_residual_label", f32, (3,)),
                                ("gt_sem_cls", "sem_cls_label", i64, ()), ("gt_box_mask", "box_label_mask", f32, ())):
        setattr(a, name, inp(gt[key], dt, (rows, 64) + tail))
    iou_labels = torch.empty((s, k), dtype=f32, device=dev)
    stats = torch.empty((len(STAT_KEYS),), dtype=f32, device=dev)
    workspace = torch.empty((int(_lib.lhs_pseudo_stats_workspace_bytes(s, k)),), dtype=torch.uint8, device=dev)
    a.iou_labels, a.stats, a.workspace = iou_labels.data_ptr(), stats.data_ptr(), workspace.data_ptr()
    _L.run("lhs_pseudo_stats", a, dev)
    out = {"unlabeled_iou_labels": iou_labels}
    out.update({name: stats[i] for i, name in enumerate(STAT_KEYS)})
    if assignment:  # (the first S*K int32 of the workspace, include/lhs_hip.h)
        out["unlabeled_iou_assignment"] = workspace[:4 * s * k].view(torch.int32).view(s, k).long()
    return out
