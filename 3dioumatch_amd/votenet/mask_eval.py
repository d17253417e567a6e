"""Mask AP: score label_points' per-point owners against ground-truth instances, on the device.

    raw = ScanStore.from_files(paths, "cuda:0")
    found = detect(engine, raw, config_dict)
    labels = label_points(found, raw)
    truth = PointTruth.from_scannet(data_dir, raw.names, "cuda:0")   # <scan>_ins_label.npy, <scan>_sem_label.npy
    meter = MaskAPCalculator((0.25, 0.5))
    meter.step(labels, found, truth)                                 # two launches, nothing waits for the GPU
    meter.compute_metrics(), meter.mean_iou()

The box AP (eval_helper.DeviceAPCalculator) matches boxes with iou3d_eval_match and marks with
iou3d_eval_mark.  The marking never looks at a box: it needs, per detection, the best overlap with a
ground-truth object of its class and that object's id.  Here the overlap is the IoU of two point sets,
and finding it is a pass over every raw point (include/mask_eval_hip.h, csrc/mask_eval.hip).

The rule.  Per scan s of n_s points:
  prediction  PointLabels.instance (owner row per point, -1 none), PointLabels.points (S, cap) (points
              per packed row) and the planes count, cls, score of the detections.  A row's score is
              score[row], or score[row, cls[row]] with per-class scores (label_points' key); its class
              is cls[row].
  truth       per point truth_instance int32 (1..G names an instance, <= 0 none) and truth_class int32
              (the detector's class id 0..NC-1, anything else: not a class); NC = found.num_class.
  size[s, g]      points of scan s with truth_instance == g + 1, g in [0, G)
  class[s, g]     truth_class of that instance's lowest-index point (ScanNet gives one label per
                  instance; this makes the class defined and order-free when a file does not); -1
                  where size is 0
  eligible g      size >= min_truth_points and 0 <= class < NC
  inter[s, r, g]  points with instance == r and truth_instance == g + 1
  detection r     r < min(max(count[s], 0), cap) and points[s, r] >= min_points (min_points >= 1: rows
                  label_points found ineligible own nothing and are never detections) and
                  0 <= cls[s, r] < min(NC, 64)
  iou(r, g)       float64(inter) / float64(points[s, r] + size[s, g] - inter), one correctly rounded division
  ovmax[s, r]     the largest iou(r, g) over eligible g with class[s, g] == cls[s, r]
  jmax[s, r]      the lowest such g reaching it (strict > update, as iou3d_eval_match does);
                  (-inf, -1) where there is no such g or the row is not a detection
  npos[c]         eligible truth instances of class c < 64; npos[64]: instances with
                  size >= min_truth_points whose class is outside [0, 64)
Scans never interact.  A prediction's size counts all its points, unannotated ones included.  Predictions
on truth instances of no class are false positives, as boxes on non-whitelisted objects are in the box AP.
Everything up to the one division is an integer and the division is IEEE: two runs are bit-equal, and so
are the device and `host_match_masks`, the rule in numpy and the path of a `device=None` store.

On the device: scene_mask_overlap (a clear launch, then one lane per point: integer atomics into the
size, class and intersection tables, equal keys of a wave merged first where MERGE says so) and
scene_mask_match (one wave per row).  Nothing in match_masks or MaskAPCalculator.step copies to the host
or synchronises.
"""
import os

import numpy as np
import torch

from .. import records
from . import point_labels as PL
from .detect import Detections
from .eval_det import EVAL_MAX_CLASS, _mark
from .eval_helper import DeviceAPCalculator
from .scannet_data import NYU40IDS

MASK_BLOCK = 256       # include/mask_eval_hip.h
MASK_MERGE_ROUNDS = 4  # include/mask_eval_hip.h
MAX_ENTRIES = 1 << 31  # words of the three tables
MERGE = True           # the overlap form match_masks launches: measured in profiles/mask_eval.json
NOT_A_DETECTION = EVAL_MAX_CLASS + 1


def table_entries(S, cap, G):
    """32-bit words of the three tables: S * G * (cap + 3)."""
    return int(S) * int(G) * (int(cap) + 3)


def _least(value, name):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < 1 or value >= 1 << 31:
        raise ValueError("%s must be an integer >= 1, got %r" % (name, value))
    return int(value)


# ---------------------------------------------------------------------------------- the truth
class PointTruth(object):
    """Ground-truth instances per point.  `instance`, `klass`: one 1-D integer array per scan, row for
    row with the scan's cloud (ids 1..G name an instance, <= 0 none; klass is the detector's class id,
    anything outside it: not a class).  Validated on the host and uploaded as flat (P,) int32 tensors
    (`device=None`: the host copy only).  `G` is the largest instance id over all scans."""

    def __init__(self, names, instance, klass, device):
        self.names = list(names)
        instance, klass = list(instance), list(klass)
        if not self.names or len(instance) != len(self.names) or len(klass) != len(self.names):
            raise ValueError("PointTruth: %d names, %d instance arrays, %d class arrays"
                             % (len(self.names), len(instance), len(klass)))
        ins, cls = [], []
        for name, i, k in zip(self.names, instance, klass):
            i, k = np.asarray(i), np.asarray(k)
            if i.ndim != 1 or k.ndim != 1 or i.dtype.kind not in "iu" or k.dtype.kind not in "iu":
                raise ValueError("PointTruth: scan %s: instance and class must be 1-D integer arrays, got %s %s and %s %s"
                                 % (name, i.dtype, i.shape, k.dtype, k.shape))
            if len(i) != len(k):
                raise ValueError("PointTruth: scan %s: %d instance ids for %d classes" % (name, len(i), len(k)))
            i, k = i.astype(np.int64), k.astype(np.int64)
            if len(i) and i.max() >= 1 << 31:
                raise ValueError("PointTruth: scan %s: instance id %d does not fit int32" % (name, int(i.max())))
            ins.append(np.maximum(i, 0).astype(np.int32))
            cls.append(np.where((k >= 0) & (k < 1 << 31), k, -1).astype(np.int32))
        self.count = np.array([len(i) for i in ins], np.int32)
        self.offset = np.concatenate([[0], np.cumsum(self.count, dtype=np.int64)[:-1]]).astype(np.int64)
        self.instance, self.klass = np.concatenate(ins), np.concatenate(cls)
        self.G = int(self.instance.max()) if len(self.instance) else 0
        if self.G < 1:
            raise ValueError("PointTruth: G = %d: no point of any scan names an instance (ids are 1..G)" % self.G)
        if table_entries(len(self.names), 1, self.G) > MAX_ENTRIES:
            raise ValueError("PointTruth: a scratch of %d table entries for %d scans and G = %d, at most 2^31"
                             % (table_entries(len(self.names), 1, self.G), len(self.names), self.G))
        self.device = torch.device(device) if device is not None else None
        self.dev = None
        if self.device is not None:
            up = lambda a: torch.from_numpy(a).to(self.device)  # noqa: E731
            self.dev = {"instance": up(self.instance), "klass": up(self.klass), "offset": up(self.offset),
                        "count": up(self.count)}

    def __len__(self):
        return len(self.names)

    @classmethod
    def from_scannet(cls, data_dir, names, device):
        """<name>_ins_label.npy / <name>_sem_label.npy of a prepared ScanNet folder; nyu40 ids become the
        18 classes through scannet_data.NYU40IDS, everything else -1."""
        table = np.full(int(NYU40IDS.max()) + 1, -1, np.int64)
        table[NYU40IDS] = np.arange(len(NYU40IDS))
        instance, klass = [], []
        for name in names:
            files = [os.path.join(data_dir, name + tail) for tail in ("_ins_label.npy", "_sem_label.npy")]
            for f in files:
                if not os.path.exists(f):
                    raise ValueError("PointTruth.from_scannet: scan %s: missing %s" % (name, f))
            ins, sem = np.load(files[0]), np.load(files[1]).astype(np.int64)
            instance.append(ins)
            klass.append(np.where((sem >= 0) & (sem < len(table)), table[np.clip(sem, 0, len(table) - 1)], -1))
        return cls(names, instance, klass, device)

    def check(self, store, cap=None):
        """ValueError unless `store` (a ScanStore or a PointLabels: names and count) holds these scans,
        row for row; with `cap` also where the scratch of that many rows passes 2^31 table entries."""
        if len(store.names) != len(self.names):
            raise ValueError("PointTruth.check: %d scans of truth, %d in the store" % (len(self.names), len(store.names)))
        for i, (a, b) in enumerate(zip(self.names, store.names)):
            if a != b:
                raise ValueError("PointTruth.check: scan %d is %r in the truth and %r in the store" % (i, a, b))
        for i, (a, b) in enumerate(zip(self.count, np.asarray(store.count))):
            if int(a) != int(b):
                raise ValueError("PointTruth.check: length mismatch: scan %s has %d points of truth and %d in the store"
                                 % (self.names[i], int(a), int(b)))
        if cap is not None and table_entries(len(self.names), cap, self.G) > MAX_ENTRIES:
            raise ValueError("PointTruth.check: a scratch of %d table entries (S = %d, cap = %d, G = %d), at most 2^31"
                             % (table_entries(len(self.names), cap, self.G), len(self.names), cap, self.G))


# ---------------------------------------------------------------------------------- the rule in numpy
def host_match_masks(instance, points, planes, truth, num_class, min_points=1, min_truth_points=1):
    """The rule of the module docstring in numpy.  `instance` (P,) and `points` (S, cap): label_points'
    results; `planes`: {count, cls, score} with the scans leading; `truth`: a PointTruth ->
    {ovmax (S, cap) f64, jmax (S, cap) i32, score (S, cap) f32, key (S, cap) i16, npos (65,) i64,
    inter (S, cap, G) i32, size (S, G) i32, klass (S, G) i32}."""
    min_points, min_truth_points = _least(min_points, "min_points"), _least(min_truth_points, "min_truth_points")
    NC = _least(num_class, "num_class")
    instance, points = np.asarray(instance, np.int32), np.asarray(points, np.int32)
    S, cap = points.shape
    G = truth.G
    cls, score = np.asarray(planes["cls"], np.int32), np.asarray(planes["score"], np.float32)
    rows = np.clip(np.asarray(planes["count"], np.int64), 0, cap)
    if len(truth) != S or cls.shape != (S, cap) or score.shape[:2] != (S, cap) or len(instance) != len(truth.instance):
        raise ValueError("host_match_masks: %d scans of %d rows, planes %s %s, %d points, truth of %d scans and %d points"
                         % (S, cap, cls.shape, score.shape, len(instance), len(truth), len(truth.instance)))
    NS = score.shape[2] if score.ndim == 3 else 0
    out = {"ovmax": np.full((S, cap), -np.inf), "jmax": np.full((S, cap), -1, np.int32),
           "score": np.zeros((S, cap), np.float32), "key": np.full((S, cap), NOT_A_DETECTION, np.int16),
           "npos": np.zeros(EVAL_MAX_CLASS + 1, np.int64), "inter": np.zeros((S, cap, G), np.int32),
           "size": np.zeros((S, G), np.int32), "klass": np.full((S, G), -1, np.int32)}
    for s in range(S):
        o, n = int(truth.offset[s]), int(truth.count[s])
        ti, tc, owner = truth.instance[o:o + n], truth.klass[o:o + n], instance[o:o + n]
        at = np.nonzero((ti >= 1) & (ti <= G))[0]  # the points naming an instance, in index order
        g = ti[at].astype(np.int64) - 1
        size = np.bincount(g, minlength=G)
        named, first = np.unique(g, return_index=True)  # the lowest-index point of each
        klass = np.full(G, -1, np.int64)
        klass[named] = tc[at[first]]
        both = (owner[at] >= 0) & (owner[at] < cap)
        inter = np.bincount(owner[at][both].astype(np.int64) * G + g[both], minlength=cap * G).reshape(cap, G)
        big = size >= min_truth_points
        eligible = big & (klass >= 0) & (klass < NC)
        c = cls[s].astype(np.int64)
        det = (np.arange(cap) < rows[s]) & (points[s] >= min_points) & (c >= 0) & (c < min(NC, EVAL_MAX_CLASS))
        if NS:
            det &= c < NS
            key = score[s][np.arange(cap), np.clip(c, 0, NS - 1)]
        else:
            key = score[s]
        union = points[s].astype(np.int64)[:, None] + size[None, :] - inter
        ok = det[:, None] & eligible[None, :] & (klass[None, :] == c[:, None])
        iou = np.where(ok, inter.astype(np.float64) / np.maximum(union, 1).astype(np.float64), -np.inf)
        best = np.argmax(iou, 1)  # the first of equal maxima: the lowest g
        ovmax = iou[np.arange(cap), best]
        out["ovmax"][s], out["jmax"][s] = ovmax, np.where(ovmax > -np.inf, best, -1)
        out["score"][s] = np.where(det, key, np.float32(0))
        out["key"][s] = np.where(det, c, NOT_A_DETECTION)
        out["inter"][s], out["size"][s], out["klass"][s] = inter, size, klass
        slot = np.where((klass >= 0) & (klass < EVAL_MAX_CLASS), klass, EVAL_MAX_CLASS)
        counted = big & ((slot == EVAL_MAX_CLASS) | (klass < NC))
        out["npos"] += np.bincount(slot[counted], minlength=EVAL_MAX_CLASS + 1)
    return out


# ---------------------------------------------------------------------------------- the launches
def mask_scratch_bytes(S, cap, G):
    """scene_mask_scratch_bytes"""
    from .. import _lib
    return int(_lib.lib.scene_mask_scratch_bytes(S, cap, G))


def scratch_views(scratch, S, cap, G):
    """(size (S, G), inter (S, cap, G)) int32 views of an overlap scratch (an int32 tensor)."""
    n = S * G
    return scratch[2 * n:3 * n].view(S, G), scratch[3 * n:3 * n + n * cap].view(S, cap, G)


def overlap_record(offset, count, max_blocks, instance, truth_instance, truth_class, scratch, S, cap, G, merge, clear):
    a = records.MaskOverlapArgs()
    a.S, a.cap, a.G, a.max_blocks, a.merge, a.clear = S, cap, G, max_blocks, int(bool(merge)), int(bool(clear))
    a.offset, a.count, a.instance = offset.data_ptr(), count.data_ptr(), instance.data_ptr()
    a.truth_instance, a.truth_class, a.scratch = truth_instance.data_ptr(), truth_class.data_ptr(), scratch.data_ptr()
    a.scratch_bytes = scratch.numel() * scratch.element_size()
    return a


def overlap_gpu(offset, count, max_blocks, instance, truth_instance, truth_class, S, cap, G, merge=MERGE, clear=True,
                scratch=None):
    """Launch scene_mask_overlap over flat (P,) int32 device arrays -> the scratch, an int32 tensor of
    table_entries(S, cap, G) words (it may be given, holding anything while `clear` is on)."""
    from .. import _lib
    if scratch is None:
        scratch = torch.empty(table_entries(S, cap, G), dtype=torch.int32, device=instance.device)
    _lib.run("scene_mask_overlap", overlap_record(offset, count, max_blocks, instance, truth_instance, truth_class,
                                                  scratch, S, cap, G, merge, clear), instance.device)
    return scratch


def match_record(rows, cls, score, points, scratch, G, NC, min_points, min_truth_points, out):
    S, cap = points.shape
    a = records.MaskMatchArgs()
    a.S, a.cap, a.G, a.NC, a.NS = S, cap, G, NC, score.shape[2] if score.dim() == 3 else 0
    a.min_points, a.min_truth_points = min_points, min_truth_points
    a.rows, a.cls, a.score, a.points = rows.data_ptr(), cls.data_ptr(), score.data_ptr(), points.data_ptr()
    a.scratch, a.scratch_bytes = scratch.data_ptr(), scratch.numel() * scratch.element_size()
    a.ovmax, a.jmax, a.row_score = out["ovmax"].data_ptr(), out["jmax"].data_ptr(), out["score"].data_ptr()
    a.key, a.klass, a.npos = out["key"].data_ptr(), out["klass"].data_ptr(), out["npos"].data_ptr()
    return a


MATCH_OUTPUTS = (("ovmax", torch.float64), ("jmax", torch.int32), ("score", torch.float32), ("key", torch.int16))


def match_gpu(rows, cls, score, points, scratch, G, NC, min_points=1, min_truth_points=1, out=None):
    """Launch scene_mask_match with an overlap scratch -> {ovmax, jmax, score, key (S, cap), klass (S, G),
    npos (65,) int64}.  Any of them may be given in `out` holding anything, except npos, which is ADDED to."""
    from .. import _lib
    S, cap = points.shape
    out = dict(out or {})
    for name, dtype in MATCH_OUTPUTS:
        if name not in out:
            out[name] = torch.empty((S, cap), dtype=dtype, device=points.device)
    if "klass" not in out:
        out["klass"] = torch.empty((S, G), dtype=torch.int32, device=points.device)
    if "npos" not in out:
        out["npos"] = torch.zeros(EVAL_MAX_CLASS + 1, dtype=torch.int64, device=points.device)
    _lib.run("scene_mask_match", match_record(rows, cls, score, points, scratch, G, NC, min_points, min_truth_points,
                                              out), points.device)
    return out


# ---------------------------------------------------------------------------------- the result
class MaskMatch(object):
    """match_masks' result: ovmax (S, cap) f64, jmax (S, cap) i32, score (S, cap) f32, key (S, cap) i16
    (the class, EVAL_MAX_CLASS + 1 for "not a detection"), npos (65,) i64, inter (S, cap, G) i32,
    size (S, G) i32, klass (S, G) i32: device tensors (numpy arrays on the host path)."""
    FIELDS = ("ovmax", "jmax", "score", "key", "npos", "inter", "size", "klass")

    def __init__(self, S, cap, G, values):
        self.S, self.cap, self.G = S, cap, G
        for name in self.FIELDS:
            setattr(self, name, values[name])

    def host(self):
        """{field: numpy array}: a copy per field on the device path."""
        return {n: (getattr(self, n).cpu().numpy() if torch.is_tensor(getattr(self, n)) else getattr(self, n))
                for n in self.FIELDS}


def match_masks(labels, found, truth, min_points=1, min_truth_points=1, merge=MERGE, buffers=None):
    """The best ground-truth instance of every packed row's mask (module docstring) -> MaskMatch.
    `labels`: label_points' PointLabels of `found` (a Detections or TiledDetections); `truth`: a
    PointTruth of the same scans.  On the device where labels and truth live on one; else in numpy.
    `merge` picks the overlap launch's form and does not change the result.  `buffers`: {scratch, ovmax,
    jmax, score, key, klass, npos} to use in place of fresh allocations (anything in them is
    overwritten, except npos, which is added to)."""
    min_points, min_truth_points = _least(min_points, "min_points"), _least(min_truth_points, "min_truth_points")
    if not isinstance(labels, PL.PointLabels):
        raise ValueError("match_masks: a PointLabels, got %s" % type(labels).__name__)
    if not isinstance(found, Detections):
        raise ValueError("match_masks: a Detections or a TiledDetections, got %s" % type(found).__name__)
    if not isinstance(truth, PointTruth):
        raise ValueError("match_masks: a PointTruth, got %s" % type(truth).__name__)
    S = len(labels.names)
    if list(found.names) != list(labels.names):
        raise ValueError("match_masks: the labels and the detections name different scans")
    cap, _ = PL._read_layout(found, S)
    if cap != labels.cap:
        raise ValueError("match_masks: labels of %d rows per scan, detections of %d" % (labels.cap, cap))
    truth.check(labels, cap)
    NC, G = _least(found.num_class, "found.num_class"), truth.G
    on_device = torch.is_tensor(labels.instance) and truth.dev is not None and torch.is_tensor(found.arena) and \
        truth.device == labels.instance.device == found.arena.device
    if not on_device:
        planes, h = found.planes(), labels.host()
        return MaskMatch(S, cap, G, host_match_masks(h["instance"], h["points"], planes, truth, NC, min_points,
                                                     min_truth_points))
    arena, d = found.arena, truth.dev
    if arena.dtype != torch.float32 or not arena.is_contiguous():
        raise ValueError("match_masks: the arena must be contiguous float32")

    def plane(name, dtype):
        at, shape = found.layout[name]
        flat = arena[at:at + int(np.prod(shape))]
        return (flat if dtype == torch.float32 else flat.view(dtype)).view(*shape)

    buffers = dict(buffers or {})
    scratch = overlap_gpu(d["offset"], d["count"], PL.max_blocks_of(truth.count), labels.instance, d["instance"],
                          d["klass"], S, cap, G, merge=merge, clear=True, scratch=buffers.pop("scratch", None))
    out = match_gpu(labels.rows, plane("cls", torch.int32), plane("score", torch.float32), labels.points, scratch, G, NC,
                    min_points, min_truth_points, out=buffers)
    out["size"], out["inter"] = scratch_views(scratch, S, cap, G)
    return MaskMatch(S, cap, G, out)


# ---------------------------------------------------------------------------------- the AP
class MaskAPCalculator(DeviceAPCalculator):
    """DeviceAPCalculator over masks: step() appends match_masks' slots in the parent's layout (score
    f32, key i16, ovmax f64, ground-truth id = slots so far + s * G + max(jmax, 0)); compute_metrics()
    and eval_det() are the parent's (two sorts, one iou3d_eval_mark launch, one host copy for all
    classes and thresholds).  Ground-truth instances of no class (walls, floor) are counted apart in
    `no_class`, not in the parent's out-of-range slot, which it refuses.  With numpy matches (a
    `device=None` store) the slots stay on the host and the marking is eval_det._mark per class."""

    def reset(self):
        DeviceAPCalculator.reset(self)
        self._truth_npos = None  # the match launches' accumulator, 65 slots
        self.no_class = None     # [64] of it: instances of eligible size and no class

    def step(self, labels, found, truth, min_points=1, min_truth_points=1):
        nmax = EVAL_MAX_CLASS
        if found.num_class > nmax:
            raise ValueError("MaskAPCalculator: %d classes, class ids must be 0 .. %d" % (found.num_class, nmax - 1))
        S, G = len(truth), truth.G
        if self._gt_slots + S * G >= 2 ** 31:
            raise ValueError("MaskAPCalculator: more than 2^31 ground-truth slots")
        on_device = torch.is_tensor(labels.instance) and truth.dev is not None
        if self._score and on_device != torch.is_tensor(self._score[0]):
            raise ValueError("MaskAPCalculator: host and device steps in one epoch")
        buffers = None
        if on_device:
            if self._truth_npos is None:
                dev = labels.instance.device
                self._truth_npos = torch.zeros(nmax + 1, dtype=torch.int64, device=dev)
                self._class_slots = torch.cat([torch.ones(nmax, dtype=torch.int64, device=dev),
                                               torch.zeros(1, dtype=torch.int64, device=dev)])
            buffers = {"npos": self._truth_npos}  # the launch adds to it
        m = match_masks(labels, found, truth, min_points, min_truth_points, buffers=buffers)
        if torch.is_tensor(m.ovmax):
            first_id = self._gt_slots + torch.arange(S, device=m.jmax.device).view(S, 1) * G
            gt_id = (first_id + m.jmax.clamp(min=0)).to(torch.int32)
            self._npos = self._truth_npos * self._class_slots  # the parent refuses a count in its last slot
        else:
            gt_id = (self._gt_slots + np.arange(S)[:, None] * G + np.maximum(m.jmax, 0)).astype(np.int32)
            self._truth_npos = m.npos if self._truth_npos is None else self._truth_npos + m.npos
            self._npos = self._truth_npos.copy()
            self._npos[nmax] = 0
        self.no_class = self._truth_npos[nmax]
        self._score.append(m.score.reshape(-1))
        self._key.append(m.key.reshape(-1))
        self._ovmax.append(m.ovmax.reshape(-1))
        self._gt_id.append(gt_id.reshape(-1))
        self._gt_slots += S * G
        self.scan_cnt += S
        return m

    def _evaluate(self, curves):
        if not self._score or torch.is_tensor(self._score[0]):
            return DeviceAPCalculator._evaluate(self, curves)
        score, key = np.concatenate(self._score), np.concatenate(self._key)
        ovmax, gt_id = np.concatenate(self._ovmax), np.concatenate(self._gt_id)
        out = []
        for thr in self.ap_iou_thresholds:
            r, p, a, l = {}, {}, {}, {}
            for c in range(EVAL_MAX_CLASS):
                sel, npos = key == c, int(self._npos[c])
                if not sel.any() and npos == 0:
                    continue
                if not sel.any():
                    r[c], p[c], a[c], l[c] = 0, 0, 0, 0
                    continue
                with np.errstate(all="ignore"):  # detections of a class without truth: 0 / 0, as the device
                    rec, prec, ap = _mark(score[sel], ovmax[sel], gt_id[sel], npos, thr, False)
                a[c], l[c] = ap, rec[-1]
                if curves:
                    r[c], p[c] = rec, prec
            out.append((r, p, a, l))
        return out

    def mean_iou(self):
        """The mean of ovmax over the detections that have one (a ground-truth instance of their class
        in their scan), NaN without any: one reduction and one two-word host copy of its own."""
        if not self._ovmax:
            return float("nan")
        if torch.is_tensor(self._ovmax[0]):
            ov = torch.cat(self._ovmax)
            has = torch.isfinite(ov)
            total, n = torch.stack([torch.where(has, ov, torch.zeros_like(ov)).sum(), has.sum().double()]).cpu().numpy()
        else:
            ov = np.concatenate(self._ovmax)
            has = np.isfinite(ov)
            total, n = float(ov[has].sum()), float(has.sum())
        return float(total / n) if n else float("nan")
