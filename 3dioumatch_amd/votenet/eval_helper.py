"""Prediction parsing of the evaluation path with the NMS on the device.

Host-side mirror of the reference models/ap_helper.py: predictions2corners3d :60-99 and
parse_predictions :101-222 with every combination of config keys the reference accepts: the 3-D NMS
branches the training scripts use (`use_3d_nms`, with or without `cls_nms`, optionally IoU-weighted
scores; train.py:263-275), the 2-D branch (`use_3d_nms` off: nms_2d_faster on the camera x / z
bounds with objectness scores; `cls_nms` / `use_iou_for_nms` are not consulted there, as in the
reference) and `remove_empty_box` in front of any of them.
The reference decodes every box on the host (B x K calls of get_3d_box,
utils/box_util.py:335-358) and runs utils/nms.py per scene in numpy; here the decoding is a few
batched float64 tensor ops, the NMS one kernel launch (votenet/pseudo_nms.py:nms3d_aabb_gpu) and
only the final, small Python lists are built on the host.

parse_groundtruths (:224-307) and APCalculator (:382-435) complete the evaluation loop of
train.py:evaluate_one_epoch; the average precision itself is votenet/eval_det.py (oriented-box IoU
on the device).

Both parsers are host listings of parse_predictions_device / parse_groundtruths_device, which return
device tensors without a host copy; DeviceAPCalculator consumes those and keeps the whole evaluation
on the device until one copy in compute_metrics (evaluate(..., device_ap=True) of votenet/inference.py
and votenet/iou_opt.py).

`remove_empty_box` (ap_helper.py:123-135) drops every proposal with fewer than five input points
inside its oriented box before the NMS.  The reference asks scipy for a Delaunay triangulation of
the eight corners per box; here one kernel (votenet/pseudo_nms.py:box_point_count_gpu) counts by
the closed-form test in float32 on end_points['point_clouds'] in place, and the counts' `>= 5` goes
to the NMS kernel as its validity mask, which is what running the NMS on the non-empty subset
gives.  Two differences: a point within about 1e-5 m of a face may be classified differently from
the triangulation (whose own answer there depends on qhull's tolerance), and a scene whose boxes
are all empty gives an all-zero pred_mask row where the reference stops at assert(len(pick)>0) --
imitating that would take a host round trip.
"""
import numpy as np
import torch


def _nms3d(center, size, heading, score, cls, thresh, old_type, same_class):
    """(S,n) bool keep mask; the GPU kernel (tests substitute the oracle)."""
    from .pseudo_nms import nms3d_aabb_gpu
    return nms3d_aabb_gpu(center, size, heading, score, cls, thresh, old_type, same_class)


def _count_points(points, center, size, heading):
    """(S,n) int32 points inside each box; the GPU kernel (tests substitute a host count)."""
    from .pseudo_nms import box_point_count_gpu
    return box_point_count_gpu(points, center, size, heading)


def _eval_match(det, keep, det_cls, gt, gt_valid, gt_cls, num_class):
    """(ovmax, jmax) (B,K,max(C,1)) of a batch's dense slots; the GPU kernel (tests substitute the
    oracle)."""
    from .eval_det import eval_match_gpu
    return eval_match_gpu(det, keep, det_cls, gt, gt_valid, gt_cls, num_class)


def _eval_mark(seg, ovmax, gt_id, npos, thresholds, num_gt, curves):
    """(ap, last_rec, rec, prec) of ordered detections for all classes and thresholds; the GPU
    kernel (tests substitute eval_det._mark)."""
    from .eval_det import eval_mark_gpu
    return eval_mark_gpu(seg, ovmax, gt_id, npos, thresholds, num_gt, curves)


def _nms_masked(center, size, heading, score, cls, thresh, old_type, same_class, dims, valid):
    """(S,n) bool keep mask of the NMS on the boxes with valid != 0 (None: all), dims 2 or 3; the
    GPU kernel (tests substitute a host loop)."""
    from .pseudo_nms import nms_aabb_masked_gpu
    return nms_aabb_masked_gpu(center, size, heading, score, cls, thresh, old_type, same_class,
                               dims, valid)


def corners_upright_camera(center, size64, heading64):
    """(B,K,3) f32 centres (depth frame), (B,K,3) f64 sizes (l,w,h), (B,K) f64 heading ->
    (B,K,8,3) f32 corners in the upright camera frame, vertex order and float64 arithmetic of
    get_3d_box (utils/box_util.py:335-358) on flip_axis_to_camera centres (ap_helper.py:28-35)."""
    dev = center.device
    # the vertex signs (1,1,-1,-1,1,1,-1,-1), (1,1,1,1,-1,-1,-1,-1), (1,-1,-1,1,1,-1,-1,1) from the
    # vertex number's bits: generated on the device, a tensor built from a list is a blocking copy
    v = torch.arange(8, device=dev)
    sx = (1 - 2 * ((v >> 1) & 1)).double()
    sy = (1 - 2 * ((v >> 2) & 1)).double()
    sz = (1 - 2 * ((v ^ (v >> 1)) & 1)).double()
    l, w, h = size64[..., 0:1], size64[..., 1:2], size64[..., 2:3]
    x, y, z = sx * l / 2, sy * h / 2, sz * w / 2                      # (B,K,8)
    c, s = torch.cos(heading64).unsqueeze(-1), torch.sin(heading64).unsqueeze(-1)
    cx = center[..., 0:1].double()
    cy = -center[..., 2:3].double()
    cz = center[..., 1:2].double()
    px = (c * x + 0.0 * y + s * z) + cx
    py = (0.0 * x + 1.0 * y + 0.0 * z) + cy
    pz = (-s * x + 0.0 * y + c * z) + cz
    return torch.stack([px, py, pz], dim=-1).float()


def decode_boxes(end_points, config):
    """arg-max heading / size class + residual -> (size64 (B,K,3), heading64 (B,K)), decoded in
    float64 as the reference's numpy class2size / class2angle do (ap_helper.py:77-92)."""
    h_cls = torch.argmax(end_points['heading_scores'], -1)
    h_res = torch.gather(end_points['heading_residuals'], 2, h_cls.unsqueeze(-1)).squeeze(2)
    s_cls = torch.argmax(end_points['size_scores'], -1)
    s_res = torch.gather(end_points['size_residuals'], 2,
                         s_cls.view(*s_cls.shape, 1, 1).expand(-1, -1, -1, 3)).squeeze(2)
    size64 = config.mean_size(s_res.device).double()[s_cls] + s_res.double()
    heading64 = config.class2angle_f64(h_cls, h_res)
    return size64, heading64


@torch.no_grad()
def parse_predictions_device(end_points, config_dict):
    """parse_predictions without its host listing: a dict of tensors on the end points' device,
    computed without a host copy or a synchronising op.
      corners   (B,K,8,3) f32  upright camera frame
      pred_mask (B,K) bool     the NMS verdict
      keep      (B,K) bool     pred_mask & (objectness probability > conf_thresh): the detections
      cls       (B,K) i64      arg-max class
      score     (B,K,C) f32 with `per_class_proposal`: sem_prob * obj_prob, the float32 product the
                reference forms in numpy (ap_helper.py:213-214); otherwise (B,K) f32 obj_prob
      nonempty  (B,K) i32      only with `remove_empty_box`
    The config keys and branches are parse_predictions', which lists this dict on the host."""
    config = config_dict['dataset_config']
    center = end_points['center']
    sem_probs = torch.softmax(end_points['sem_cls_scores'], dim=-1)
    pred_sem_cls = torch.argmax(end_points['sem_cls_scores'], -1)
    obj_prob = torch.softmax(end_points['objectness_scores'], dim=-1)[:, :, 1]
    size64, heading64 = decode_boxes(end_points, config)
    corners = corners_upright_camera(center, size64, heading64)

    nonempty = None
    if config_dict.get('remove_empty_box', False):
        count = _count_points(end_points['point_clouds'], center.contiguous(), size64, heading64)
        nonempty = (count >= 5).to(torch.int32)

    scores = obj_prob
    use_3d = bool(config_dict.get('use_3d_nms', True))
    same_class = use_3d and bool(config_dict.get('cls_nms', False))
    if same_class and config_dict.get('use_iou_for_nms', False):
        iou = torch.sigmoid(end_points['iou_scores'])
        if iou.shape[2] > 1:
            iou = torch.gather(iou, 2, pred_sem_cls.unsqueeze(-1))
        scores = scores * iou.squeeze(-1)
    if use_3d and nonempty is None:
        pred_mask = _nms3d(center.contiguous(), size64, heading64, scores.contiguous(), pred_sem_cls,
                           config_dict['nms_iou'], config_dict['use_old_type_nms'], same_class)
    else:
        pred_mask = _nms_masked(center.contiguous(), size64, heading64, scores.contiguous(),
                                pred_sem_cls, config_dict['nms_iou'],
                                config_dict['use_old_type_nms'], same_class, 3 if use_3d else 2,
                                nonempty)
    out = {'corners': corners, 'pred_mask': pred_mask,
           'keep': pred_mask & (obj_prob > config_dict['conf_thresh']), 'cls': pred_sem_cls,
           'score': (sem_probs * obj_prob.unsqueeze(-1)) if config_dict['per_class_proposal'] else obj_prob}
    if nonempty is not None:
        out['nonempty'] = nonempty
    return out


@torch.no_grad()
def parse_predictions(end_points, config_dict):
    """-> batch_pred_map_cls: per scene a list of (class, corners (8,3) ndarray, confidence), as
    ap_helper.parse_predictions returns it; also fills end_points['pred_mask'] (B,K),
    end_points['batch_pred_map_cls'] and, with `remove_empty_box`, end_points['nonempty_box_mask']
    (B,K).  The host listing of parse_predictions_device."""
    config = config_dict['dataset_config']
    dev = parse_predictions_device(end_points, config_dict)
    # one device->host copy of the small results, then the reference's list layout
    if 'nonempty' in dev:
        end_points['nonempty_box_mask'] = dev['nonempty'].cpu().numpy().astype(np.float64)
    keep = dev['keep'].cpu().numpy()
    # (B,K) float64 numpy array of 0/1 like the reference's (ap_helper.py:141-155), so that
    # consumers such as dump_helper index / multiply it the same way
    end_points['pred_mask'] = dev['pred_mask'].cpu().numpy().astype(np.float64)
    corners_h = dev['corners'].cpu().numpy()
    score_h = dev['score'].cpu().numpy()
    cls_h = dev['cls'].cpu().numpy()
    batch = []
    for i in range(keep.shape[0]):
        js = np.nonzero(keep[i])[0]
        if config_dict['per_class_proposal']:
            cur = [(ii, corners_h[i, j], score_h[i, j, ii])
                   for ii in range(config.num_class) for j in js]
        else:
            cur = [(int(cls_h[i, j]), corners_h[i, j], score_h[i, j]) for j in js]
        batch.append(cur)
    end_points['batch_pred_map_cls'] = batch
    return batch


@torch.no_grad()
def parse_groundtruths_device(end_points, config_dict):
    """parse_groundtruths without its host listing: corners (B,G,8,3) f32 of all B x MAX_NUM_OBJ
    labels decoded in one batched float64 pass, valid (B,G) bool = box_label_mask == 1 and cls
    (B,G) i64, on the labels' device and without a host copy."""
    config = config_dict['dataset_config']
    center = end_points['center_label'][:, :, 0:3].float()
    size64 = config.mean_size(center.device).double()[end_points['size_class_label'].long()] + \
        end_points['size_residual_label'].double()
    heading64 = config.class2angle_f64(end_points['heading_class_label'].long(),
                                       end_points['heading_residual_label'].float())
    return {'corners': corners_upright_camera(center, size64, heading64),
            'valid': end_points['box_label_mask'] == 1, 'cls': end_points['sem_cls_label'].long()}


@torch.no_grad()
def parse_groundtruths(end_points, config_dict):
    """-> batch_gt_map_cls: per scene a list of (class, corners (8,3) float32 ndarray) of the boxes
    with box_label_mask == 1 (ap_helper.py:224-307: groundtruths2corners3d + parse_groundtruths);
    the host listing of parse_groundtruths_device."""
    dev = parse_groundtruths_device(end_points, config_dict)
    corners = dev['corners'].cpu().numpy()
    mask = dev['valid'].cpu().numpy()
    sem = dev['cls'].cpu().numpy()
    batch = [[(int(sem[i, j]), corners[i, j]) for j in np.nonzero(mask[i])[0]]
             for i in range(mask.shape[0])]
    end_points['batch_gt_map_cls'] = batch
    return batch


class APCalculator(object):
    """ap_helper.py:382-435: accumulates per-scan predictions / ground truths, then one
    eval_det (votenet/eval_det.py) per compute_metrics with the oriented-box IoU."""

    def __init__(self, ap_iou_thresh=0.25, class2type_map=None, device=None):
        self.ap_iou_thresh = ap_iou_thresh
        self.class2type_map = class2type_map
        self.device = device
        self.reset()

    def step(self, batch_pred_map_cls, batch_gt_map_cls):
        bsize = len(batch_pred_map_cls)
        assert bsize == len(batch_gt_map_cls)
        for i in range(bsize):
            self.gt_map_cls[self.scan_cnt] = batch_gt_map_cls[i]
            self.pred_map_cls[self.scan_cnt] = batch_pred_map_cls[i]
            self.scan_cnt += 1

    def compute_metrics(self):
        from .eval_det import eval_det
        rec, prec, ap = eval_det(self.pred_map_cls, self.gt_map_cls, ovthresh=self.ap_iou_thresh,
                                 device=self.device)
        name = lambda key: self.class2type_map[key] if self.class2type_map else str(key)  # noqa: E731
        ret_dict = {}
        for key in sorted(ap.keys()):
            ret_dict['%s Average Precision' % name(key)] = ap[key]
        ret_dict['mAP'] = np.mean(list(ap.values()))
        rec_list = []
        for key in sorted(ap.keys()):
            last = rec[key][-1] if np.ndim(rec[key]) and len(rec[key]) else 0
            ret_dict['%s Recall' % name(key)] = last
            rec_list.append(last)
        ret_dict['AR'] = np.mean(rec_list)
        return ret_dict

    def reset(self):
        self.gt_map_cls = {}    # {scan_id: [(classname, bbox)]}
        self.pred_map_cls = {}  # {scan_id: [(classname, bbox, score)]}
        self.scan_cnt = 0


class DeviceAPCalculator(object):
    """APCalculator for the outputs of parse_predictions_device / parse_groundtruths_device, all
    thresholds at once and without a host round trip per batch.

    step() launches one match kernel (include/iou3d_hip.h iou3d_eval_match: every (proposal,
    ground-truth box) IoU of the batch once, the best box per (proposal, class) slot) and appends the
    batch's slots to a list of device tensors; nothing in it waits for the GPU.  compute_metrics()
    concatenates, orders the slots by (class, score descending, (scan, proposal) order -- two stable
    device sorts), marks true / false positives and integrates the precision envelope for every
    class and threshold in one launch (iou3d_eval_mark) and makes ONE device->host copy.  The
    results are eval_det's: the reported classes are those with a detection or a ground-truth box; a
    class with ground truth and no detection reports 0 / 0 / 0; one with detections and no ground
    truth NaN (0 / 0), as the host path does.

    The store is dense: every (scene, proposal, class) slot of a batch is kept -- score f32, class
    key i16, ovmax f64, ground-truth id i32 = 18 bytes -- whether the proposal survived the NMS or
    not, because dropping the others needs either their count on the host or an unordered atomic
    counter.  That is about 0.6 MB per ScanNet batch (8 x 256 x 18 slots) and about 0.3 GB for the
    5050 scans of SUN RGB-D val (x 256 x 10).  Class ids are 0 .. 63.  There is no CPU path."""

    def __init__(self, ap_iou_thresholds=(0.25, 0.5), class2type_map=None):
        self.ap_iou_thresholds = tuple(float(t) for t in ap_iou_thresholds)
        if not self.ap_iou_thresholds:
            raise ValueError("DeviceAPCalculator: at least one IoU threshold")
        self.class2type_map = class2type_map
        self.reset()

    def reset(self):
        self._score, self._key, self._ovmax, self._gt_id = [], [], [], []
        self._npos = None      # (MAX_CLASS + 1) i64 on the device: boxes per class, [-1]: ids out of range
        self._gt_slots = 0     # ground-truth slots so far = the next batch's first ground-truth id
        self.scan_cnt = 0

    def step(self, pred, gt):
        """pred: parse_predictions_device's dict, gt: parse_groundtruths_device's, of one batch."""
        from .eval_det import EVAL_MAX_CLASS as nmax
        keep, score, valid = pred['keep'], pred['score'], gt['valid']
        b, k = keep.shape
        g = valid.shape[1]
        if valid.shape[0] != b:
            raise ValueError("DeviceAPCalculator.step: %d scenes of predictions, %d of ground truth"
                             % (b, valid.shape[0]))
        c = score.shape[2] if score.dim() == 3 else 0
        if self._gt_slots + b * g >= 2 ** 31:
            raise ValueError("DeviceAPCalculator: more than 2^31 ground-truth slots")
        dev = keep.device
        ovmax, jmax = _eval_match(pred['corners'], keep, pred['cls'], gt['corners'], valid, gt['cls'], c)
        if c > 0:
            key = torch.arange(c, device=dev).expand(b, k, c)
        else:
            key = pred['cls'].unsqueeze(-1)
            key = torch.where((key >= 0) & (key < nmax), key, nmax)
        key = torch.where(keep.unsqueeze(-1), key, nmax + 1).to(torch.int16)   # nmax + 1: not a detection
        first_id = self._gt_slots + torch.arange(b, device=dev).view(b, 1, 1) * g
        self._score.append(score.reshape(-1).float())
        self._key.append(key.reshape(-1))
        self._ovmax.append(ovmax.reshape(-1))
        self._gt_id.append((first_id + jmax.clamp(min=0)).to(torch.int32).reshape(-1))
        if self._npos is None:
            self._npos = torch.zeros(nmax + 1, dtype=torch.int64, device=dev)
        gcls = gt['cls']
        gkey = torch.where((gcls >= 0) & (gcls < nmax), gcls, nmax)
        self._npos.scatter_add_(0, gkey.reshape(-1), valid.reshape(-1).to(torch.int64))
        self._gt_slots += b * g
        self.scan_cnt += b

    def _evaluate(self, curves):
        """-> per threshold (rec, prec, ap, last) dicts keyed by class; rec / prec hold the curves
        only with `curves` (more host copies), `last` the recall at the class's last detection."""
        from .eval_det import EVAL_MAX_CLASS as nmax
        nt = len(self.ap_iou_thresholds)
        if not self._score:
            return [({}, {}, {}, {}) for _ in range(nt)]
        score, key = torch.cat(self._score), torch.cat(self._key)
        ovmax, gt_id = torch.cat(self._ovmax), torch.cat(self._gt_id)
        dev = score.device
        # (class, score descending, insertion): a stable sort by score, then a stable sort by class
        by_score = torch.sort(-score, stable=True).indices
        key_sorted, by_key = torch.sort(key[by_score], stable=True)
        order = by_score[by_key]
        seg = torch.searchsorted(key_sorted, torch.arange(nmax + 2, dtype=torch.int16, device=dev))
        thr = torch.cat([torch.full((1,), t, dtype=torch.float64, device=dev) for t in self.ap_iou_thresholds])
        ap, last, rec, prec = _eval_mark(seg[:nmax + 1].contiguous(), ovmax[order], gt_id[order],
                                         self._npos[:nmax].contiguous(), thr, self._gt_slots, curves)
        host = torch.cat([ap.reshape(-1), last.reshape(-1), seg.double(), self._npos.double()]).cpu().numpy()
        ap_h, last_h = host[:nt * nmax].reshape(nt, nmax), host[nt * nmax:2 * nt * nmax].reshape(nt, nmax)
        seg_h = host[2 * nt * nmax:2 * nt * nmax + nmax + 2].astype(np.int64)
        npos_h = host[2 * nt * nmax + nmax + 2:].astype(np.int64)
        if seg_h[nmax + 1] > seg_h[nmax] or npos_h[nmax] > 0:
            raise ValueError("DeviceAPCalculator: class ids must be 0 .. %d" % (nmax - 1))
        if curves:
            rec, prec = rec.cpu().numpy(), prec.cpu().numpy()
        out = []
        for t in range(nt):
            r, p, a, l = {}, {}, {}, {}
            for c in range(nmax):
                s0, s1 = int(seg_h[c]), int(seg_h[c + 1])
                if s1 == s0 and npos_h[c] == 0:
                    continue
                if s1 == s0:
                    r[c], p[c], a[c], l[c] = 0, 0, 0, 0
                    continue
                a[c], l[c] = ap_h[t, c], last_h[t, c]
                if curves:
                    r[c], p[c] = rec[t, s0:s1], prec[t, s0:s1]
            out.append((r, p, a, l))
        return out

    def eval_det(self):
        """-> per threshold (rec, prec, ap) dicts keyed by class, as eval_det.eval_det returns them."""
        return [(r, p, a) for r, p, a, _ in self._evaluate(True)]

    def compute_metrics(self):
        """-> per threshold the dict APCalculator.compute_metrics returns."""
        name = lambda key: self.class2type_map[key] if self.class2type_map else str(key)  # noqa: E731
        ret = []
        for _, _, ap, last in self._evaluate(False):
            ret_dict = {}
            for key in sorted(ap.keys()):
                ret_dict['%s Average Precision' % name(key)] = ap[key]
            ret_dict['mAP'] = np.mean(list(ap.values()))
            for key in sorted(ap.keys()):
                ret_dict['%s Recall' % name(key)] = last[key]
            ret_dict['AR'] = np.mean([last[key] for key in sorted(ap.keys())])
            ret.append(ret_dict)
        return ret


class EvalLossMeter(object):
    """The loss statistics of an evaluation epoch (train.py:395-414, :427): the sum over batches of each of
    the 20 keys losses.get_loss fills, on the device, and the number of batches on the host.

    step() runs the criterion on one batch's end_points (predictions and labels).  On the fused path the
    statistics kernel adds the batch's values to the sums itself (votenet_eval_loss' accum); on the tensor
    path one torch.stack is added to the same vector.  Neither reads a value on the host: nothing in step()
    waits for the device.  result() makes ONE device->host copy and divides by the batch count -- a plain
    mean of per-batch means, not weighted by batch size, as in the reference."""

    def __init__(self, device):
        from .fused_loss import EV_COUNT
        self.device = torch.device(device)
        self.accum = torch.zeros(EV_COUNT, dtype=torch.float32, device=self.device)
        self.batches = 0

    def step(self, end_points, dataset_config):
        """(loss, end_points) of losses.get_loss on this batch, its statistics added to the sums."""
        from . import fused_loss, losses
        losses.check_eval_labels(end_points)
        if 'iou_scores' not in end_points:
            raise ValueError("EvalLossMeter.step: the end_points have no 'iou_scores' (iou_loss is one of the "
                             "logged keys)")
        dev = end_points['center'].device
        if dev != self.accum.device:
            raise ValueError("EvalLossMeter.step: end_points on %s, the meter on %s" % (dev, self.accum.device))
        if fused_loss.eval_supported(end_points):
            out = fused_loss.get_loss_fused(end_points, dataset_config, accum=self.accum)
        else:
            out = losses.get_loss(end_points, dataset_config)
            values = [end_points[key].float() for key in losses.EVAL_STAT_KEYS]
            values.append(end_points['objectness_label'].sum().float())
            self.accum += torch.stack(values)
        self.batches += 1
        return out

    def result(self):
        """{key: epoch mean} of the 20 keys plus 'mean_loss' (= the mean detection_loss)."""
        from .losses import EVAL_STAT_KEYS
        if self.batches == 0:
            raise ValueError("EvalLossMeter.result: no batch was evaluated")
        host = self.accum.cpu().numpy().astype(np.float64) / self.batches
        stats = {key: float(host[i]) for i, key in enumerate(EVAL_STAT_KEYS)}
        stats['mean_loss'] = stats['detection_loss']
        return stats
