"""The supervised loss as two kernel launches around the per-scene IoU kernel (binding of
include/loss_hip.h; csrc/votenet_loss.hip, csrc/loss_core.h).

`get_labeled_loss_fused` fills the same end_points keys as votenet/losses.py:get_labeled_loss
(the mirror of models/loss_helper_labeled.py:300-370) from one statistics vector, and the gradient
of the loss with respect to every head output comes out of the same launch: the autograd node
below just hands those buffers over, scaled by the incoming gradient of `loss`.  Only
`end_points['loss']` (= 'detection_loss') is differentiable; the other entries are logging values.
`get_pseudo_detection_loss_fused` is the same for the consistency loss on pseudo labels (the kernels'
consistency mode), `get_semi_loss_fused` both losses of the semi-supervised step on one gradient buffer.

`get_loss_fused` is the test-time criterion (losses.get_loss, models/loss_helper.py:222-291) on the eval kernels:
forward only, four launches, and optionally the running sums of an epoch added on the device.

Written once each: the differentiable inputs and their gradients (_HEADS, _grad_layout), the pass that
fills VnLossArgs and launches (_loss_pass, both modes), the backward (_split_grads), the pseudo labels
(_pseudo_labels), the end_points entries of each loss (_fill_supervised, _fill_unlabeled) and the
switch of the consistency kernels (consistency_supported).
"""
import collections
import ctypes
import importlib
import math
import os

import torch

from ..records import VnLossArgs, VnLossTensor

_PRED = ("agg_xyz", "obj", "center", "h_scores", "h_resn", "s_scores", "s_resn", "sem", "iou",
         "iou_jit", "seed_xyz", "vote_xyz", "jit_center", "jit_size", "jit_heading")

# The differentiable inputs, in the order the gradients lie in a flat buffer: (VnLossArgs prediction
# field, its gradient field, end_points key, shape of ONE scene's gradient as the kernels write it;
# names are looked up in _dims).  The consistency mode has the first seven.
_HEADS = (
    ("obj", "g_obj", 'objectness_scores', ("K", 2)),
    ("center", "g_center", 'center', ("K", 3)),
    ("h_scores", "g_h_scores", 'heading_scores', ("K", "NH")),
    ("h_resn", "g_h_resn", 'heading_residuals_normalized', ("K", "NH")),
    ("s_scores", "g_s_scores", 'size_scores', ("K", "NS")),
    ("s_resn", "g_s_resn", 'size_residuals_normalized', ("K", "NS", 3)),
    ("sem", "g_sem", 'sem_cls_scores', ("K", "NC")),
    ("iou", "g_iou", 'iou_scores', ("K", "NI")),
    ("iou_jit", "g_iou_jit", 'iou_scores_jitter', ("K", "NI")),   # no jitter: no floats, gradient None
    ("vote_xyz", "g_vote", 'vote_xyz', ("S*VF", 3)),
)
_FIELDS = tuple(row[0] for row in _HEADS)
_GRADS = tuple(row[1] for row in _HEADS)
_CONSISTENCY_GRADS = _GRADS[1:7]  # (g_obj is written too, as zeros: objectness is a statistic there)


(ST_LOSS, ST_VOTE, ST_OBJ, ST_CENTER, ST_HCLS, ST_HREG, ST_SCLS, ST_SREG, ST_SEM, ST_BOX, ST_IOU,
 ST_JIT, ST_POS_RATIO, ST_NEG_RATIO, ST_OBJ_ACC, ST_OBJ_COUNT, ST_CLS_ACC, ST_PRED_IOU,
 ST_PRED_IOU_OBJ, ST_IOU_ACC, ST_IOU_ACC_OBJ, ST_JIT_ACC, ST_JIT_ACC_OBJ, ST_COUNT) = range(24)

_STAT_KEYS = {
    'vote_loss': ST_VOTE, 'objectness_loss': ST_OBJ, 'center_loss': ST_CENTER,
    'heading_cls_loss': ST_HCLS, 'heading_reg_loss': ST_HREG, 'size_cls_loss': ST_SCLS,
    'size_reg_loss': ST_SREG, 'sem_cls_loss': ST_SEM, 'box_loss': ST_BOX, 'iou_loss': ST_IOU,
    'pos_ratio': ST_POS_RATIO, 'neg_ratio': ST_NEG_RATIO, 'obj_acc': ST_OBJ_ACC,
    'obj_count': ST_OBJ_COUNT, 'cls_acc': ST_CLS_ACC, 'pred_iou_value': ST_PRED_IOU,
    'pred_iou_obj_value': ST_PRED_IOU_OBJ, 'iou_acc': ST_IOU_ACC, 'iou_acc_obj': ST_IOU_ACC_OBJ,
}
_JITTER_KEYS = {'jitter_iou_loss': ST_JIT, 'jitter_iou_acc': ST_JIT_ACC,
                'jitter_iou_acc_obj': ST_JIT_ACC_OBJ}


def enabled():
    return os.environ.get("VOTENET_FUSED_LOSS", "1") != "0"


_HOST_BUILD = None  # tests: ctypes handle of tests/loss_host.cpp (same arithmetic, host pointers)
_EVAL_HOST_BUILD = None  # tests: the same of tests/eval_loss_host.cpp (the test-time criterion)


def available(device):
    return device.type == "cuda" or _HOST_BUILD is not None


def _launch(name, args, device):
    if device.type != "cuda":
        if _HOST_BUILD is None:
            raise RuntimeError("the fused loss runs on the GPU only (no CPU path)")
        rc = getattr(_HOST_BUILD, name.replace("votenet_loss", "host_loss"))(ctypes.byref(args))
        assert rc == 0
        return
    from .. import _lib
    _lib.run(name, args, device)


def _scratch_floats(args, device):
    if device.type != "cuda":
        if _HOST_BUILD is None:
            raise RuntimeError("the fused loss runs on the GPU only (no CPU path)")
        return int(_HOST_BUILD.host_loss_scratch_floats(ctypes.byref(args)))
    from .. import _lib
    return int(_lib.lib.votenet_loss_scratch_floats(ctypes.byref(args)))


def _scene_iou(boxes, gt_boxes):
    """(best IoU (B,P) f32, first best same-scene GT index (B,P) i32)."""
    if boxes.is_cuda:
        cuda = importlib.import_module("pcdet.ops.iou3d_nms.iou3d_nms_cuda")
        best = torch.empty(boxes.shape[:2], dtype=torch.float32, device=boxes.device)
        idx = torch.empty(boxes.shape[:2], dtype=torch.int32, device=boxes.device)
        cuda.scene_best_iou3d_gpu(boxes, gt_boxes, best, idx)
        return best, idx
    from .losses import _scene_best_iou
    best, idx = _scene_best_iou(boxes, gt_boxes)
    return best.float().contiguous(), idx.int().contiguous()


def _view(t):
    s = list(t.stride()) + [0] * (4 - t.dim())
    return VnLossTensor(t.data_ptr(), s[0], s[1], s[2] if t.dim() > 2 else 0, s[3] if t.dim() > 3 else 0)


_Grad = collections.namedtuple("_Grad", "per size shape")  # floats per scene, floats, shape of n scenes


def _dims(preds):
    """What the gradient shapes are functions of, from the head outputs {prediction field: tensor}."""
    vote = preds.get("vote_xyz")
    return {"K": preds["center"].shape[1], "NH": preds["h_scores"].shape[2], "NS": preds["s_scores"].shape[2],
            "NC": preds["sem"].shape[2], "NI": preds["iou"].shape[2] if "iou" in preds else 1,
            "S*VF": 0 if vote is None else vote.shape[1], "jitter": preds.get("iou_jit") is not None}


def _grad_layout(dims, n):
    """{gradient field: _Grad} of n scenes, in _GRADS order."""
    layout = {}
    for _, name, _, shape in _HEADS:
        shape = tuple(dims.get(d, d) for d in shape)
        per = 0 if name == "g_iou_jit" and not dims["jitter"] else math.prod(shape)
        layout[name] = _Grad(per, n * per, (n,) + shape if per else (0,))
    return layout


def _carve(flat, layout, names):
    """{gradient field: device address} of consecutive pieces of `flat`, in the order of `names`."""
    dest, at = {}, flat.data_ptr()
    for name in names:
        dest[name] = at
        at += 4 * layout[name].size
    return dest


def _split_grads(flat, g, layout, names=_GRADS):
    """flat * g as one gradient per row of _HEADS (None: not among `names`, or no floats); `flat` holds
    the pieces of `names` back to back."""
    scaled = flat * g
    out, at = [], 0
    for name in _GRADS:
        size = layout[name].size if name in names else 0
        out.append(scaled[at:at + size].view(layout[name].shape) if size else None)
        at += size
    return tuple(out)


_F32, _I64 = torch.float32, torch.int64
# (VnLossArgs field = end_points key of the supervised loss, key among the pseudo labels, dtype)
_LABELS = (('center_label', 'center', _F32), ('box_label_mask', 'mask', _F32),
           ('heading_class_label', 'heading_class', _I64), ('heading_residual_label', 'heading_residual', _F32),
           ('size_class_label', 'size_class', _I64), ('size_residual_label', 'size_residual', _F32),
           ('sem_cls_label', 'sem_cls', _I64), ('vote_label', None, _F32), ('vote_label_mask', None, _I64))
# (VnLossArgs tensor field, key) of the inputs without a gradient; the consistency mode has the first
_INPUTS = (("agg_xyz", 'aggregated_vote_xyz'), ("seed_xyz", 'seed_xyz'))
_JITTER_INPUTS = (("jit_center", 'jitter_center'), ("jit_size", 'jitter_size'), ("jit_heading", 'jitter_heading'))


def _fill_args(consistency, src, config, heads, grad_scale=1.0):
    """VnLossArgs with the sizes, labels and predictions of one pass filled in (see _loss_pass for `src` and
    `heads`) -> (args, tensors the struct points into, ptr() to add more, _dims, device)."""
    preds = dict(zip(_FIELDS, heads))
    center, has_jitter = preds["center"], preds.get("iou_jit") is not None
    dev, (nb, k) = center.device, center.shape[:2]
    dims = _dims(preds)
    a = VnLossArgs()
    a.B, a.K, a.G = nb, k, src['center' if consistency else 'center_label'].shape[1]
    a.NH, a.NS, a.NC, a.NI = dims["NH"], dims["NS"], dims["NC"], dims["NI"]
    if not consistency:
        a.S, a.N = src['seed_xyz'].shape[1], src['vote_label'].shape[1]
        a.VF = dims["S*VF"] // a.S
    a.has_jitter, a.consistency, a.grad_scale = int(has_jitter), int(consistency), float(grad_scale)
    keep = []  # tensors whose storage the struct points into

    def ptr(t):
        keep.append(t)
        return t.data_ptr()
    for field, key, dt in _LABELS:
        if consistency and key is None:
            continue  # (no votes in this mode)
        t = src[key if consistency else field]
        if consistency and (t.dtype != dt or t.shape[0] != nb):
            raise RuntimeError("pseudo label %s must be %s with %d scenes" % (key, dt, nb))
        if t.dtype != dt:
            raise RuntimeError("%s must be %s" % (field, dt))
        setattr(a, field, ptr(t.contiguous()))
    if not consistency:
        seed_inds = src['seed_inds']
        if seed_inds.dtype != torch.int32 or seed_inds.stride(1) != 1:
            seed_inds = seed_inds.int().contiguous()
        a.seed_inds, a.seed_inds_stride = ptr(seed_inds), seed_inds.stride(0)
    a.mean_size = ptr(config.mean_size(dev).contiguous())
    for name, key in _INPUTS[:1] if consistency else _INPUTS + (_JITTER_INPUTS if has_jitter else ()):
        preds[name] = src[key]
    for name in _PRED:
        t = preds.get(name)
        if t is None:
            t = center  # not read in this mode (or without jitter)
        if t.dtype != torch.float32 or t.device != dev:
            raise RuntimeError("%s must be a float32 tensor on %s" % (name, dev))
        keep.append(t)
        setattr(a, name, _view(t))
    return a, keep, ptr, dims, dev


def _loss_pass(consistency, src, config, heads, grad_dest=None, grad_scale=1.0):
    """The launches of one mode over the scenes of `heads`.

    supervised: decode -> scene IoU -> forward_backward; `src` is end_points (_LABELS, seed_inds, _INPUTS,
    _JITTER_INPUTS; their first scenes are read), `heads` the ten tensors of _HEADS cut to the labeled scenes
    (iou_scores_jitter None: no jitter).  consistency: forward_backward alone with S = VF = N = 0, NI = 1;
    `src` holds the pseudo labels and 'aggregated_vote_xyz', `heads` the first seven tensors.
    grad_dest: {gradient field: device address} to write the gradient rows somewhere the caller owns (a buffer
    both modes share); None: a buffer of its own.  Returns (stats, objectness_label, objectness_mask,
    object_assignment, pred_bbox or None, that buffer or None, its _grad_layout)."""
    a, keep, ptr, dims, dev = _fill_args(consistency, src, config, heads, grad_scale)
    nb, k, has_jitter = a.B, a.K, bool(a.has_jitter)
    f32 = dict(dtype=torch.float32, device=dev)
    pred_bbox = None
    if not consistency:
        boxes = torch.empty((nb, 2 * k if has_jitter else k, 7), **f32)
        gt_boxes = torch.empty((nb, a.G, 7), **f32)
        a.boxes, a.gt_boxes = ptr(boxes), ptr(gt_boxes)
        _launch("votenet_loss_decode", a, dev)
        iou_lab, iou_assign = _scene_iou(boxes, gt_boxes)
        a.iou_lab, a.iou_assign = ptr(iou_lab), ptr(iou_assign)
        pred_bbox = boxes[:, :k]
    out = {"stats": torch.empty(ST_COUNT, **f32),
           "objectness_label": torch.empty((nb, k), dtype=torch.int64, device=dev),
           "objectness_mask": torch.empty((nb, k), **f32),
           "object_assignment": torch.empty((nb, k), dtype=torch.int64, device=dev),
           "gt_nearest": torch.empty((nb, a.G), dtype=torch.int32, device=dev)}
    for name, t in out.items():
        setattr(a, name, ptr(t))
    a.partials = ptr(torch.empty(max(1, _scratch_floats(a, dev)), **f32))
    layout = _grad_layout(dims, nb)
    names = _GRADS[:7] if consistency else _GRADS
    flat = None
    if grad_dest is None:
        flat = torch.empty(sum(layout[name].size for name in names), **f32)  # every element is written by the kernel
        grad_dest = _carve(flat, layout, names)
        keep.append(flat)
    for name in names:
        setattr(a, name, grad_dest[name])
    _launch("votenet_loss_forward_backward", a, dev)
    return (out["stats"], out["objectness_label"], out["objectness_mask"], out["object_assignment"], pred_bbox,
            flat, layout)


def _labeled_pass(end_points, config, nb, *heads, **grads):
    """_loss_pass in its supervised mode; `heads` are cut to the nb labeled scenes"""
    out = _loss_pass(False, end_points, config, heads, **grads)
    return out[:5] + (out[5:],)


def _consistency_pass(labels, config, agg_xyz, *heads, **grads):
    """_loss_pass in its consistency mode on the scenes of `heads` (no pred_bbox)"""
    out = _loss_pass(True, dict(labels, aggregated_vote_xyz=agg_xyz), config, heads, **grads)
    return out[:4] + (out[5:],)


def _only_loss_differentiable(ctx, *others):
    ctx.mark_non_differentiable(*others)
    # (the other outputs' gradients are never read: no zeros are made for them)
    ctx.set_materialize_grads(False)


class _FusedLabeledLoss(torch.autograd.Function):
    """stats, labels <- launches; backward: the stored gradients times d(loss)."""

    @staticmethod
    def forward(ctx, end_points, config, *heads):
        stats, label, mask, assignment, pred_bbox, (ctx.flat, ctx.layout) = _labeled_pass(
            end_points, config, heads[1].shape[0], *heads)
        _only_loss_differentiable(ctx, label, mask, assignment, pred_bbox)
        return stats, label, mask, assignment, pred_bbox

    @staticmethod
    def backward(ctx, g_stats, *unused):
        return (None, None) + _split_grads(ctx.flat, g_stats[ST_LOSS], ctx.layout)


class _FusedConsistencyLoss(torch.autograd.Function):
    """The consistency loss on pseudo labels (losses_unlabeled.get_pseudo_detection_loss) with the
    kernels of the supervised loss (VnLossArgs.consistency = 1): ONE call, two launches, where the
    tensor version is ~90 small kernels forward and as many backward."""

    @staticmethod
    def forward(ctx, labels, config, agg_xyz, *heads):
        stats, label, mask, assignment, (ctx.flat, ctx.layout) = _consistency_pass(labels, config, agg_xyz, *heads)
        _only_loss_differentiable(ctx, label, mask, assignment)
        return stats, label, mask, assignment

    @staticmethod
    def backward(ctx, g_stats, *unused):
        behind = ctx.flat[ctx.layout["g_obj"].size:]  # (the objectness rows are zeros: no gradient)
        return (None, None, None) + _split_grads(behind, g_stats[ST_LOSS], ctx.layout, _CONSISTENCY_GRADS)[:7]


class _FusedSemiLoss(torch.autograd.Function):
    """detection_loss + weight * unlabeled_detection_loss of the semi-supervised step
    (train.py:327-333) as ONE autograd node: the supervised loss' launches on the labeled scenes and
    the consistency mode's on the unlabeled ones write the rows of ONE gradient buffer per head
    output (the consistency rows already scaled by `weight`: VnLossArgs.grad_scale), so the backward
    is one multiplication -- where two nodes on two slices of every head output cost a zero-fill
    and a copy per slice (slice_backward) and an addition per output."""

    @staticmethod
    def forward(ctx, end_points, config, ln, weight, labels, *heads):
        preds = dict(zip(_FIELDS, heads))
        layout = _grad_layout(_dims(preds), preds["center"].shape[0])
        # (the IoU / vote rows of the unlabeled scenes stay zero)
        flat = torch.zeros(sum(g.size for g in layout.values()), dtype=torch.float32, device=preds["center"].device)
        base = _carve(flat, layout, _GRADS)
        stats_l, lab_l, mask_l, assign_l, pred_bbox, _ = _labeled_pass(
            end_points, config, ln, *[t if t is None else t[:ln] for t in heads], grad_dest=base)
        dest_u = {name: base[name] + 4 * ln * layout[name].per for name in _GRADS[:7]}
        stats_u, lab_u, mask_u, assign_u, _ = _consistency_pass(
            labels, config, end_points['aggregated_vote_xyz'][ln:], *[t[ln:] for t in heads[:7]],
            grad_dest=dest_u, grad_scale=weight)
        total = stats_l[ST_LOSS] + stats_u[ST_LOSS] * weight
        ctx.flat, ctx.layout = flat, layout
        _only_loss_differentiable(ctx, stats_l, stats_u, lab_l, mask_l, assign_l, pred_bbox, lab_u, mask_u, assign_u)
        return total, stats_l, stats_u, lab_l, mask_l, assign_l, pred_bbox, lab_u, mask_u, assign_u

    @staticmethod
    def backward(ctx, g_total, *unused):
        return (None, None, None, None, None) + _split_grads(ctx.flat, g_total, ctx.layout)


_CONSISTENCY_KEYS = {
    'unlabeled_objectness_loss': ST_OBJ, 'unlabeled_pos_ratio': ST_POS_RATIO,
    'unlabeled_neg_ratio': ST_NEG_RATIO, 'unlabeled_center_loss': ST_CENTER,
    'unlabeled_heading_cls_loss': ST_HCLS, 'unlabeled_heading_reg_loss': ST_HREG,
    'unlabeled_size_cls_loss': ST_SCLS, 'unlabeled_size_reg_loss': ST_SREG,
    'unlabeled_sem_cls_loss': ST_SEM, 'unlabeled_box_loss': ST_BOX,
}


def supported(end_points, supervised_inds):
    return (supervised_inds is None or isinstance(supervised_inds, slice)) and \
        'iou_scores' in end_points and end_points['center'].dim() == 3


def consistency_supported(end_points):
    """the consistency kernels may run (VOTENET_FUSED_LOSS=0 or VOTENET_FUSED_CONSISTENCY=0: tensor operations)"""
    return (enabled() and os.environ.get("VOTENET_FUSED_CONSISTENCY", "1") != "0"
            and available(end_points['center'].device) and end_points['center'].dim() == 3)


def semi_loss_supported(end_points, labeled_num):
    return (consistency_supported(end_points) and os.environ.get("VOTENET_FUSED_SEMI_LOSS", "1") != "0"
            and 'iou_scores' in end_points and 0 < labeled_num < end_points['center'].shape[0])


def _head_outputs(end_points, cut, count=len(_HEADS)):
    """cut(head output) of the first `count` rows of _HEADS (iou_scores_jitter None: no jitter)"""
    return [cut(end_points[key]) if key != 'iou_scores_jitter' or 'jitter_center' in end_points else None
            for _, _, key, _ in _HEADS[:count]]


def _pseudo_labels(end_points):
    """{pseudo-label key of _LABELS: end_points['unlabeled_' + field]}; the centres of empty slots are masked as the
    reference does in place (loss_helper_unlabeled.py:150-152), and stored back"""
    mask = end_points['unlabeled_box_label_mask']
    center = end_points['unlabeled_center_label'][:, :, 0:3]
    center = torch.where((1 - mask).unsqueeze(-1).bool(), torch.full_like(center, -1000), center)
    end_points['unlabeled_center_label'] = center
    labels = {key: end_points['unlabeled_' + field] for field, key, _ in _LABELS if key}
    labels['mask'] = mask.float()
    return labels


def _fill_supervised(end_points, stats, objectness_label, objectness_mask, object_assignment, pred_bbox):
    log = stats.detach()
    for key, i in _STAT_KEYS.items():
        end_points[key] = log[i]
    if 'jitter_center' in end_points:
        for key, i in _JITTER_KEYS.items():
            end_points[key] = log[i]
    end_points['objectness_label'] = objectness_label
    end_points['objectness_mask'] = objectness_mask
    end_points['object_assignment'] = object_assignment
    end_points['pred_bbox'] = pred_bbox
    end_points['detection_loss'] = stats[ST_LOSS]


def _fill_unlabeled(end_points, stats, objectness_label, objectness_mask, object_assignment):
    log = stats.detach()
    for key, i in _CONSISTENCY_KEYS.items():
        end_points[key] = log[i]
    end_points['unlabeled_objectness_label'] = objectness_label
    end_points['unlabeled_objectness_mask'] = objectness_mask
    end_points['unlabeled_object_assignment'] = object_assignment
    end_points['unlabeled_detection_loss'] = stats[ST_LOSS]


def get_labeled_loss_fused(end_points, dataset_config, supervised_inds=None):
    """Same contract as losses.get_labeled_loss for `supervised_inds` None (every scene) or
    slice(0, n) (labeled scenes first)."""
    nb = end_points['center'].shape[0] if supervised_inds is None else int(supervised_inds.stop)
    heads = _head_outputs(end_points, lambda t: t if t.shape[0] == nb else t[:nb])
    _fill_supervised(end_points, *_FusedLabeledLoss.apply(end_points, dataset_config, *heads))
    loss = end_points['loss'] = end_points['detection_loss']
    return loss, end_points


def get_pseudo_detection_loss_fused(end_points, labeled_num, config):
    """Same contract as losses_unlabeled.get_pseudo_detection_loss (same end_points keys)."""
    tail = slice(labeled_num, None)
    labels = _pseudo_labels(end_points)
    _fill_unlabeled(end_points, *_FusedConsistencyLoss.apply(
        labels, config, end_points['aggregated_vote_xyz'][tail], *_head_outputs(end_points, lambda t: t[tail], 7)))
    return end_points['unlabeled_detection_loss'], end_points


def get_semi_loss_fused(end_points, config, labeled_num, weight):
    """(loss, end_points) with loss = detection_loss + weight * unlabeled_detection_loss and every key
    get_labeled_loss_fused and get_pseudo_detection_loss_fused fill; the pseudo labels
    (`unlabeled_*_label`, `unlabeled_box_label_mask`) are already in end_points."""
    labels = _pseudo_labels(end_points)
    total, stats_l, stats_u, lab_l, mask_l, assign_l, pred_bbox, lab_u, mask_u, assign_u = _FusedSemiLoss.apply(
        end_points, config, int(labeled_num), float(weight), labels, *_head_outputs(end_points, lambda t: t))
    _fill_supervised(end_points, stats_l, lab_l, mask_l, assign_l, pred_bbox)
    _fill_unlabeled(end_points, stats_u, lab_u, mask_u, assign_u)
    end_points['loss'] = total
    return total, end_points


# ---- the test-time criterion ----------------------------------------------------------------------------
EV_COUNT = 21  # include/loss_hip.h VN_EV_COUNT: losses.EVAL_STAT_KEYS in order, then the positive count
EV_LOSS, EV_OBJ_COUNT = 0, 20


def eval_supported(end_points):
    """the eval kernels may run: the gate of get_labeled_loss (VOTENET_FUSED_LOSS, an IoU head, (B,K,C) head
    outputs) on the GPU (tests: the host build)"""
    on_device = end_points['center'].device.type == "cuda" or _EVAL_HOST_BUILD is not None
    return enabled() and supported(end_points, None) and on_device


def _launch_eval(name, a, device, *more):
    """votenet_eval_loss_decode(args) / votenet_eval_loss(args, stats, accum) on the current stream (tests:
    the host build's host_eval_loss*)"""
    more = [None if t is None else ctypes.c_void_p(t.data_ptr()) for t in more]
    if device.type != "cuda":
        if _EVAL_HOST_BUILD is None:
            raise RuntimeError("the fused loss runs on the GPU only (no CPU path)")
        rc = getattr(_EVAL_HOST_BUILD, name.replace("votenet_", "host_"))(ctypes.byref(a), *more)
        assert rc == 0
        return
    from .. import _lib
    _lib.run(name, a, device, *more)


def _eval_pass(src, config, heads, size_residuals, accum=None):
    """decode -> scene IoU -> terms -> statistics of the test-time criterion over every scene of `heads` (the
    tensors of _HEADS, iou_scores_jitter None); `src` as in _loss_pass, `size_residuals` (B,K,NS,3) the
    unnormalised residuals the boxes are decoded from.  accum: EV_COUNT floats the statistics are added to.
    Returns (stats, objectness_label, objectness_mask, object_assignment, iou_labels, pred_bbox)."""
    a, keep, ptr, dims, dev = _fill_args(False, src, config, heads)
    nb, k = a.B, a.K
    if size_residuals.dtype != torch.float32 or size_residuals.device != dev:
        raise RuntimeError("size_residuals must be a float32 tensor on %s" % (dev,))
    keep.append(size_residuals)
    a.jit_size = _view(size_residuals)
    if accum is not None and (accum.dtype != torch.float32 or accum.device != dev or accum.numel() != EV_COUNT
                              or not accum.is_contiguous()):
        raise RuntimeError("accum must be %d contiguous float32 values on %s" % (EV_COUNT, dev))
    f32 = dict(dtype=torch.float32, device=dev)
    boxes, gt_boxes = torch.empty((nb, k, 7), **f32), torch.empty((nb, a.G, 7), **f32)
    a.boxes, a.gt_boxes = ptr(boxes), ptr(gt_boxes)
    _launch_eval("votenet_eval_loss_decode", a, dev)
    iou_lab, _ = _scene_iou(boxes, gt_boxes)
    a.iou_lab = ptr(iou_lab)
    out = {"objectness_label": torch.empty((nb, k), dtype=torch.int64, device=dev),
           "objectness_mask": torch.empty((nb, k), **f32),
           "object_assignment": torch.empty((nb, k), dtype=torch.int64, device=dev)}
    for name, t in out.items():
        setattr(a, name, ptr(t))
    scratch = (_scratch_floats(a, dev) if dev.type == "cuda" or _EVAL_HOST_BUILD is None
               else int(_EVAL_HOST_BUILD.host_eval_loss_scratch_floats(ctypes.byref(a))))
    a.partials = ptr(torch.empty(max(1, scratch), **f32))
    stats = torch.empty(EV_COUNT, **f32)
    _launch_eval("votenet_eval_loss", a, dev, stats, accum)
    return stats, out["objectness_label"], out["objectness_mask"], out["object_assignment"], iou_lab, boxes


@torch.no_grad()
def get_loss_fused(end_points, dataset_config, accum=None):
    """Same contract as losses.get_loss: the 20 keys of losses.EVAL_STAT_KEYS as views of one statistics vector,
    'loss', the objectness labels / mask / assignment, 'iou_labels' and 'pred_bbox'.  accum: a device vector of
    EV_COUNT floats the kernel adds this batch's statistics to (votenet_eval_loss), no host round trip."""
    from .losses import EVAL_STAT_KEYS
    heads = [end_points[key].detach() if key != 'iou_scores_jitter' else None for _, _, key, _ in _HEADS]
    stats, label, mask, assignment, iou_labels, pred_bbox = _eval_pass(
        end_points, dataset_config, heads, end_points['size_residuals'].detach(), accum)
    for i, key in enumerate(EVAL_STAT_KEYS):
        end_points[key] = stats[i]
    end_points['objectness_label'] = label
    end_points['objectness_mask'] = mask
    end_points['object_assignment'] = assignment
    end_points['iou_labels'] = iou_labels
    end_points['pred_bbox'] = pred_bbox
    end_points['loss'] = end_points['detection_loss']
    return end_points['loss'], end_points
