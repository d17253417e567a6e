"""Inputs and float64 truth for the test-time criterion's tests (tests/test_eval_loss.py,
tests/test_eval_loss_gpu.py; no network, no package import).

  build(name, no_positive)   loss_kernel_cases.build(name) without the jitter inputs, plus 'size_residuals' (the
                             unnormalised residuals the boxes are decoded from: fp32(s_resn * mean_size), and 0.25 m
                             more on every other proposal of the last scene, as after a box optimisation: a decode
                             from s_resn misses those boxes by 0.25 m) and, in
                             every case with K >= 3 and G >= 2, three planted proposals in the last scene:
      (a) `ka`: a proposal whose aggregated vote is 0.12 m from the raw centre of the scene's EMPTY slots (the
          origin, what the loaders pad with) and metres from every real centre: positive for
          models/loss_helper.py (:86-92, raw centre labels), negative for loss_helper_labeled.py (empty slots
          at -1000); its assignment is the FIRST empty slot (an exact tie between identical points);
      (b) `kb`: a positive proposal whose predicted class differs from the class of its best-IoU box AND from
          the class of its assigned box: with NI > 1 the IoU channel of :208-210 is not the training one (the
          two channels' scores are +8 and -8), and the proposal is a wrong classification among the positives;
      (c) `kc`: a negative proposal whose predicted class is the class of its assigned box: counted by cls_acc
          (:188-189, unmasked), not by cls_acc_obj (:190-192).
                             The margin rule is loss_kernel_cases.margins' (1e-4 around 0.3 / 0.6, 1e-5 relative
                             between the two nearest candidates), recomputed for the RAW centre distances; the
                             empty slots of a scene count as one candidate (their tie is exact: first index).
  reference(name, ...)       models/loss_helper.py:25-291 in float64, written from its formulas: labels, the 20
                             logged statistics and the positive count, the decoded boxes with their bounds.
"""
import functools

import numpy as np

import loss_kernel_cases as base
from loss_kernel_cases import EPS, F32, FAR, NEAR, SHIFT

STAT_KEYS = ('detection_loss', 'vote_loss', 'objectness_loss', 'center_loss', 'heading_cls_loss',
             'heading_reg_loss', 'size_cls_loss', 'size_reg_loss', 'sem_cls_loss', 'box_loss', 'iou_loss',
             'pos_ratio', 'neg_ratio', 'obj_acc', 'cls_acc', 'cls_acc_obj', 'pred_iou_value',
             'pred_iou_obj_value', 'iou_acc', 'iou_acc_obj', 'obj_count')
# what the two criteria compute differently because of the planted proposals: (a) one more positive, (c) the
# unmasked cls_acc, the masked iou_loss, and -- NI > 1 only -- (b) the IoU channel of one positive
PLANTED_KEYS = ('obj_count', 'cls_acc', 'iou_loss')
PLANTED_KEYS_CLASS_IOU = ('iou_acc_obj',)


def _raw_distances(c, b):
    """(K, candidates) squared distances of scene b's aggregated votes to its RAW centre labels, float64"""
    cols = base._candidates(c, b)
    d = np.float64
    return ((c["agg_xyz"][b].astype(d)[:, None] - c["center_label"][b].astype(d)[None, cols]) ** 2).sum(-1)


def raw_margins(c):
    bad = []
    for b in range(c["B"]):
        first, second, _ = base._two_smallest(_raw_distances(c, b))
        dist = np.sqrt(first + 1e-6)
        off = base._tied(first, second) | (np.abs(dist - NEAR) < 1e-4) | (np.abs(dist - FAR) < 1e-4)
        bad += [(b, int(k)) for k in np.flatnonzero(off)]
    return bad


def _assign_raw(c):
    """first arg-min over the raw centre labels, float64: (B, K)"""
    d = np.float64
    d2 = ((c["agg_xyz"].astype(d)[:, :, None] - c["center_label"].astype(d)[:, None]) ** 2).sum(-1)
    return np.argmin(d2, -1), d2


@functools.lru_cache(maxsize=None)
def build(name, no_positive=False):
    src = base.build(name, False, no_positive)
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in src.items()
         if k not in ("iou_jit", "jitter_center", "jitter_size", "jitter_heading")}
    B, K, G, NC = c["B"], c["K"], c["G"], c["NC"]
    c["jitter"] = False
    c["iou_lab"] = np.ascontiguousarray(src["iou_lab"][:, :K])
    c["iou_assign"] = np.ascontiguousarray(src["iou_assign"][:, :K])
    c["size_residuals"] = (c["s_resn"] * c["mean_size"][None, None]).astype(F32)
    c["size_residuals"][-1, ::2] += F32(0.25)  # the last scene's even proposals: not what s_resn would decode to
    c["planted"] = None
    if K >= 3 and G >= 2 and not no_positive:
        ps = src["plants"]["scene"]
        taken = {src["plants"][k] for k in ("kq", "pa", "pb", "pc")}
        train = base.reference(name)
        empty = np.flatnonzero(c["box_label_mask"][ps] != 1)
        assert len(empty) and not c["center_label"][ps, empty].any(), "the planted scene needs an empty slot at 0"
        neg = [k for k in np.flatnonzero((train["objectness_label"][ps] == 0) & (train["objectness_mask"][ps] == 1))
               if k not in taken]
        pos = [k for k in np.flatnonzero(train["objectness_label"][ps] == 1) if k not in taken]
        ka, kc, kb = int(neg[1]), int(neg[2]), int(pos[0])
        c["agg_xyz"][ps, ka] = (0.1, 0.05, -0.04)          # (a)
        assign, _ = _assign_raw(c)
        cls = c["sem_cls_label"][ps]
        wrong = next(j for j in range(NC) if j not in (cls[c["iou_assign"][ps, kb]], cls[assign[ps, kb]]))
        c["sem"][ps, kb] = -5.0
        c["sem"][ps, kb, wrong] = 30.0                      # (b), and the positive half of (c)
        if c["NI"] > 1:  # the two channels far apart: sigmoid ~1 at the predicted class, ~0 at the training one
            c["iou"][ps, kb, wrong], c["iou"][ps, kb, cls[c["iou_assign"][ps, kb]]] = 8.0, -8.0
        c["sem"][ps, kc] = -5.0
        c["sem"][ps, kc, cls[assign[ps, kc]]] = 30.0        # (c)
        c["planted"] = dict(scene=ps, ka=ka, kb=kb, kc=kc, first_empty=int(empty[0]))
    for attempt in range(8):
        bad = raw_margins(c)
        if not bad:
            break
        for b, k in bad:
            c["agg_xyz"][b, k] += SHIFT
    assert not raw_margins(c) and not base.margins(c)
    return c


def _huber(x):
    a = np.abs(x)
    return np.where(a <= 1, 0.5 * x * x, a - 0.5)


def _logsumexp(x):
    m = x.max(-1, keepdims=True)
    return (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))[..., 0]


def _take(v, idx):
    """v (B, G[, 3]) at idx (B, K)"""
    return np.take_along_axis(v, idx.reshape(idx.shape + (1,) * (v.ndim - 2)), 1)


@functools.lru_cache(maxsize=None)
def reference(name, no_positive=False):
    """float64 labels and statistics (key -> float) of models/loss_helper.py:get_loss on a case, and the
    decoded boxes with their rounding-count bounds; computed once and shared (read-only)."""
    c = build(name, no_positive)
    d = np.float64
    B, K, S, VF, NH, NI = c["B"], c["K"], c["S"], c["VF"], c["NH"], c["NI"]
    f = lambda k: c[k].astype(d)  # noqa: E731
    total = float(B * K)
    st = {}
    # compute_vote_loss :25-70
    pair = base._vote_distances(c)
    vmask = np.take_along_axis(c["vote_label_mask"], c["seed_inds"].astype(np.int64), 1).astype(d)
    st["vote_loss"] = (pair.min(-1) * vmask).sum() / (vmask.sum() + 1e-6)
    # compute_objectness_loss :72-113: raw centre labels, first index
    assign, d2 = _assign_raw(c)
    dist = np.sqrt(np.take_along_axis(d2, assign[..., None], -1)[..., 0] + 1e-6)
    label = dist < NEAR
    omask = ((dist < NEAR) | (dist > FAR)).astype(d)
    obj = label.astype(d)
    cnt, msum = obj.sum(), omask.sum()
    scores = f("obj")
    ce = np.where(label, 0.8, 0.2) * (_logsumexp(scores) - np.where(label, scores[..., 1], scores[..., 0]))
    st["objectness_loss"] = (ce * omask).sum() / (msum + 1e-6)
    st["obj_acc"] = (((scores[..., 1] > scores[..., 0]) == label) * omask).sum() / (msum + 1e-6)
    st["pos_ratio"] = cnt / total
    st["neg_ratio"] = msum / total - st["pos_ratio"]
    st["obj_count"] = cnt
    pos_mean = lambda v: (v * obj).sum() / (cnt + 1e-6)  # noqa: E731
    # compute_box_and_sem_cls_loss :115-220
    dc = ((f("center")[:, :, None] - f("center_label")[:, None]) ** 2).sum(-1)
    bmask = f("box_label_mask")
    st["center_loss"] = pos_mean(dc.min(2)) + (dc.min(1) * bmask).sum() / (bmask.sum() + 1e-6)

    def cross_entropy(s, cls):
        return _logsumexp(s) - np.take_along_axis(s, cls[..., None], -1)[..., 0]

    hl = _take(c["heading_class_label"], assign)
    st["heading_cls_loss"] = pos_mean(cross_entropy(f("h_scores"), hl))
    target = _take(f("heading_residual_label"), assign) / (np.pi / NH)
    st["heading_reg_loss"] = pos_mean(_huber(np.take_along_axis(f("h_resn"), hl[..., None], -1)[..., 0] - target))
    sl = _take(c["size_class_label"], assign)
    st["size_cls_loss"] = pos_mean(cross_entropy(f("s_scores"), sl))
    s_target = _take(f("size_residual_label"), assign) / f("mean_size")[sl]
    s_pred = np.take_along_axis(f("s_resn"), sl[..., None, None], 2)[:, :, 0]
    st["size_reg_loss"] = pos_mean(_huber(s_pred - s_target).mean(-1))
    cl = _take(c["sem_cls_label"], assign)
    st["sem_cls_loss"] = pos_mean(cross_entropy(f("sem"), cl))
    pred_cls = np.argmax(c["sem"], -1)
    match = (pred_cls == cl).astype(d)
    st["cls_acc"] = match.sum() / total
    st["cls_acc_obj"] = pos_mean(match)
    st["box_loss"] = (0.1 * st["heading_cls_loss"] + st["heading_reg_loss"] + 0.1 * st["size_cls_loss"]
                      + st["size_reg_loss"] + st["center_loss"])
    lab = f("iou_lab")
    st["pred_iou_value"] = lab.sum() / total
    st["pred_iou_obj_value"] = pos_mean(lab)
    p = 1.0 / (1.0 + np.exp(-f("iou")))
    p = np.take_along_axis(p, pred_cls[..., None], -1)[..., 0] if NI > 1 else p[..., 0]
    x = p - lab
    st["iou_acc"] = np.abs(x).sum() / total
    st["iou_acc_obj"] = pos_mean(np.abs(x))
    st["iou_loss"] = pos_mean(_huber(x))
    # get_loss :276-281
    st["detection_loss"] = 10 * (st["vote_loss"] + 0.5 * st["objectness_loss"] + st["box_loss"]
                                 + 0.1 * st["sem_cls_loss"] + st["iou_loss"])
    # the boxes: loss_helper_iou.py:64-88 with size = mean + size_residuals (one rounding)
    dec = base.decode_reference(c)
    sc = np.argmax(c["s_scores"], -1)
    mean = f("mean_size")[sc]
    res = np.take_along_axis(f("size_residuals"), sc[..., None, None], 2)[:, :, 0]
    size = mean + res
    assert (np.abs(size) > 1e-5).all(), "a decoded size next to 0"
    clamped = size <= 0
    dec["boxes"][:, :, 3:6] = np.where(clamped, d(F32(1e-6)), size)
    dec["boxes_bound"][:, :, 3:6] = np.where(clamped, 0.0, EPS * (np.abs(mean) + np.abs(res)))
    dec["clamped"] = clamped
    return dict(stats={k: float(v) for k, v in st.items()}, objectness_label=label.astype(np.int64),
                objectness_mask=omask, object_assignment=assign, **dec)
