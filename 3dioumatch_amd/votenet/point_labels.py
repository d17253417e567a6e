"""Per-point instance labels from packed detections, on the device: which box owns each raw point.

    raw = ScanStore.from_files(paths, "cuda:0")
    found = detect(engine, VoxelStore.from_store(raw, 0.05), config_dict)
    labels = label_points(found, raw)                       # boxes found on the thinned copy, points of the raw scan
    tiled = detect_tiled(engine, TileStore.from_store(raw, 8.0), config_dict, seam_nms=True)
    labels = label_points(tiled, tiled.store.source)        # tiles are not recentred: the boxes hold for the parent
    labels.instance, labels.semantic, labels.points         # device tensors; labels[i], by_name, points_of, save read
    labels.index()                                          # the points of each row as lists (votenet/point_index.py)

The reference answers "which points lie in this box" with extract_pc_in_box3d (sunrgbd/sunrgbd_utils.py:215-224),
a scipy Delaunay hull per box on the host (models/ap_helper.py:123-135).  Here the test is the closed form
of csrc/box_points.hip with one lane per point (include/point_labels_hip.h).

The rule.  `found` is a Detections or a TiledDetections; only its planes count, cls, score and box are
read, `cap` rows per scan.  Rows at or past `count` are never read.
  frame     of a packed row, from box = (cx, cy, cz, l, w, h, heading): c = float32(cos(float64(heading))),
            s = float32(sin(float64(heading))), hl, hw, hh = float32(float64(size) / 2).
  inside    float32, every operation rounded, no contraction: d = p - centre, x' = c dx - s dy,
            z' = s dx + c dy; the point is inside iff |x'| <= hl and |z'| <= hw and |dz| <= hh (faces inclusive).
  key       score[row], or score[row, cls[row]] with per-class scores (the seam NMS's key).
  eligible  row < count, every frame value finite, l, w, h > 0, the key not NaN and >= max(min_score, 0)
            (and, with per-class scores, 0 <= cls < NC).  An ineligible row owns nothing.
  owner     of a point: among the eligible rows that contain it the one with the largest 64-bit rank word;
            low word 0xFFFFFFFF - row (ties go to the lowest row), high word bits(|key|) with
            prefer="score", 0xFFFFFFFF - bits(v), v = (l * w) * h in float32 rounded each time, with
            prefer="smallest" (a mug on a table goes to the mug).  No such row: -1.
  results   instance (P,) int32 flat over the store's rows: the owner; semantic: cls[owner] or -1;
            points (S, cap): the points each row owns.  Scans never interact; everything is an integer,
            so two runs are bit-equal.

On the device: scene_detections_frames (one thread per row: frame, rank, cls, a bounding radius, points
zeroed) and scene_points_label (grid (blocks of the longest scan, S), LABEL_BLOCK points per workgroup,
the eligible rows staged through LDS LABEL_BOX_CHUNK at a time; with the cull a row is staged only if
its bounding sphere reaches the bounding box of the workgroup's points -- exact, see
csrc/point_labels.hip).  Nothing in label_points copies to the host or synchronises; the first read of
the result makes ONE copy.  `host_label_points` restates the rule in numpy and is the path of a
`device=None` store or of an arena on another device.
"""
import os

import numpy as np
import torch

from .. import records
from .detect import MAX_K, Detections
from .scan_data import ScanStore

LABEL_BLOCK = 256      # include/point_labels_hip.h
LABEL_BOX_CHUNK = 256  # include/point_labels_hip.h
PREFER = ("score", "smallest")
CULL = True            # label_points' default: measured in profiles/label_points.json
HOST_POINTS = 1 << 16  # points per pass of the numpy restatement


def _prefer(prefer):
    if prefer not in PREFER:
        raise ValueError("prefer must be one of %s, got %r" % (PREFER, prefer))
    return PREFER.index(prefer)


def _min_score(min_score):
    try:
        m = float(min_score)
    except (TypeError, ValueError):
        m = float("nan")
    if not np.isfinite(m):
        raise ValueError("min_score must be finite, got %r" % (min_score,))
    return m


# ---------------------------------------------------------------------------------- the rule in numpy
def host_frames(planes, prefer="score", min_score=0.0, frames=None):
    """The frames launch in numpy: {frames (S, cap, 8) float32, rank (S, cap) uint64 (0: ineligible),
    cls (S, cap) int32, reach (S, cap) float64: sqrt(hl^2 + hw^2 + hh^2)}, all zero past count.
    `planes`: {count, cls, score, box} with the scans leading.  `frames`: frames to take in place of
    the ones computed here (the device's, whose cos and sin may differ in the last bit)."""
    mode, least = _prefer(prefer), max(_min_score(min_score), 0.0)
    cls = np.asarray(planes["cls"], np.int32)
    S, cap = cls.shape
    live = np.arange(cap)[None, :] < np.clip(np.asarray(planes["count"], np.int64), 0, cap)[:, None]
    box = np.where(live[..., None], np.asarray(planes["box"], np.float32).reshape(S, cap, 7), np.float32(0))
    score = np.asarray(planes["score"], np.float32)
    with np.errstate(all="ignore"):
        if frames is None:
            ang = box[..., 6].astype(np.float64)
            half = (box[..., 3:6].astype(np.float64) / 2).astype(np.float32)
            frames = np.concatenate([np.cos(ang).astype(np.float32)[..., None], np.sin(ang).astype(np.float32)[..., None],
                                     box[..., 0:3], half], -1)
        frames = np.where(live[..., None], np.asarray(frames, np.float32).reshape(S, cap, 8), np.float32(0))
        ok = live & np.isfinite(frames).all(-1) & (box[..., 3:6] > 0).all(-1)
        if score.ndim == 3:
            ok &= (cls >= 0) & (cls < score.shape[2])
            key = np.take_along_axis(score, np.clip(cls, 0, score.shape[2] - 1)[..., None].astype(np.int64), 2)[..., 0]
        else:
            key = score
        key = np.where(ok, key, np.float32(0))  # rows past count are not read
        ok &= key.astype(np.float64) >= least   # false for a NaN key
        if mode == 0:
            high = np.abs(key).view(np.uint32)
        else:
            high = np.uint32(0xFFFFFFFF) - ((box[..., 3] * box[..., 4]) * box[..., 5]).view(np.uint32)
        low = np.uint32(0xFFFFFFFF) - np.arange(cap, dtype=np.uint32)[None, :]
        rank = (high.astype(np.uint64) << np.uint64(32)) | low.astype(np.uint64)
        half = frames[..., 5:8].astype(np.float64)
        reach = np.sqrt((half[..., 0] * half[..., 0] + half[..., 1] * half[..., 1]) + half[..., 2] * half[..., 2])
    return {"frames": np.ascontiguousarray(frames), "rank": np.where(ok, rank, np.uint64(0)),
            "cls": np.where(live, cls, np.int32(0)), "reach": np.where(ok, reach, 0.0)}


def host_inside(xyz, frame):
    """(n,) bool: the float32 membership test of one frame (c, s, cx, cy, cz, hl, hw, hh)."""
    c, s, cx, cy, cz, hl, hw, hh = (np.float32(v) for v in frame)
    dx, dy, dz = xyz[:, 0] - cx, xyz[:, 1] - cy, xyz[:, 2] - cz
    xr = c * dx - s * dy   # numpy rounds every float32 operation: no contraction
    zr = s * dx + c * dy
    return (np.abs(xr) <= hl) & (np.abs(zr) <= hw) & (np.abs(dz) <= hh)


def host_label_points(planes, clouds, prefer="score", min_score=0.0, frames=None):
    """The rule of the module docstring in numpy, without any cull: `planes` = {count, cls, score, box}
    with the scans leading (Detections.planes()), `clouds` = one (n, 3) or (n, 6) array per scan ->
    {instance (P,), semantic (P,) int32 flat over the clouds, points (S, cap) int32, frames (S, cap, 8)}."""
    f = host_frames(planes, prefer, min_score, frames)
    S, cap = f["rank"].shape
    if len(clouds) != S:
        raise ValueError("host_label_points: %d clouds for %d scans of detections" % (len(clouds), S))
    instance, semantic = [], []
    points = np.zeros((S, cap), np.int32)
    for s, cloud in enumerate(clouds):
        xyz = np.ascontiguousarray(np.asarray(cloud, np.float32)[:, 0:3])
        rows = np.nonzero(f["rank"][s])[0]
        best = np.zeros(len(xyz), np.uint64)
        with np.errstate(all="ignore"):
            for p0 in range(0, len(xyz), HOST_POINTS):
                part, top = xyz[p0:p0 + HOST_POINTS], best[p0:p0 + HOST_POINTS]
                for r in rows:
                    rank = f["rank"][s, r]
                    np.maximum(top, np.where(host_inside(part, f["frames"][s, r]), rank, np.uint64(0)), out=top)
        owner = np.where(best != 0, (np.uint64(0xFFFFFFFF) - (best & np.uint64(0xFFFFFFFF))).astype(np.int64), -1)
        instance.append(owner.astype(np.int32))
        semantic.append(np.where(owner >= 0, f["cls"][s][np.maximum(owner, 0)], -1).astype(np.int32))
        points[s] = np.bincount(owner[owner >= 0], minlength=cap)
    return {"instance": np.concatenate(instance), "semantic": np.concatenate(semantic), "points": points,
            "frames": f["frames"]}


# ---------------------------------------------------------------------------------- the launches
def label_scratch_bytes(S, cap):
    """scene_points_label_scratch_bytes"""
    from .. import _lib
    return int(_lib.lib.scene_points_label_scratch_bytes(S, cap))


def frames_record(count, cls, score, box, K, prefer, min_score, frames, points, scratch):
    S, cap = cls.shape
    a = records.DetectionsFramesArgs()
    a.S, a.K, a.cap, a.NC, a.prefer = S, K, cap, score.shape[2] if score.dim() == 3 else 0, _prefer(prefer)
    a.min_score = _min_score(min_score)
    a.count, a.cls, a.score, a.box = count.data_ptr(), cls.data_ptr(), score.data_ptr(), box.data_ptr()
    a.frames, a.points, a.scratch = frames.data_ptr(), points.data_ptr(), scratch.data_ptr()
    a.scratch_bytes = scratch.numel() * scratch.element_size()
    return a


def frames_gpu(count, cls, score, box, K, prefer="score", min_score=0.0, frames=None, points=None, scratch=None):
    """Launch scene_detections_frames over device planes count (S,) int32, cls (S, cap) int32, score
    (S, cap) or (S, cap, NC) float32, box (S, cap, 7) float32 (views of an arena will do) ->
    (frames (S, cap, 8) float32, points (S, cap) int32 zeroed, scratch: int64 words).  The three outputs
    may be given; they may hold anything."""
    from .. import _lib
    S, cap = cls.shape
    dev = cls.device
    if frames is None:
        frames = torch.empty((S, cap, 8), dtype=torch.float32, device=dev)
    if points is None:
        points = torch.empty((S, cap), dtype=torch.int32, device=dev)
    if scratch is None:
        scratch = torch.empty(label_scratch_bytes(S, cap) // 8, dtype=torch.int64, device=dev)
    _lib.run("scene_detections_frames",
             frames_record(count, cls, score, box, K, prefer, min_score, frames, points, scratch), dev)
    return frames, points, scratch


def scratch_views(scratch, S, cap):
    """(rank (S, cap) int64 bit patterns, cls (S, cap) int32, radius (S, cap) float32) of a frames scratch."""
    n = S * cap
    rank = scratch[:n].view(S, cap)
    rest = scratch[n:2 * n].view(torch.int32)
    return rank, rest[:n].view(S, cap), rest[n:2 * n].view(torch.float32).view(S, cap)


def label_record(cloud, offset, count, max_blocks, rows, frames, scratch, K, cull, instance, semantic, points):
    S, cap = points.shape
    a = records.PointsLabelArgs()
    a.S, a.C, a.K, a.cap, a.cull, a.max_blocks = S, cloud.shape[1], K, cap, int(bool(cull)), max_blocks
    a.cloud, a.offset, a.count, a.rows = cloud.data_ptr(), offset.data_ptr(), count.data_ptr(), rows.data_ptr()
    a.frames, a.scratch = frames.data_ptr(), scratch.data_ptr()
    a.scratch_bytes = scratch.numel() * scratch.element_size()
    a.instance, a.semantic, a.points = instance.data_ptr(), semantic.data_ptr(), points.data_ptr()
    return a


def label_gpu(cloud, offset, count, max_blocks, rows, frames, scratch, K, points, cull=CULL, instance=None,
              semantic=None):
    """Launch scene_points_label over the scans of a flat (P, C) device cloud with what frames_gpu
    returned (`points` is added to) -> (instance (P,), semantic (P,)) int32; both may be given."""
    from .. import _lib
    P = cloud.shape[0]
    if instance is None:
        instance = torch.empty(P, dtype=torch.int32, device=cloud.device)
    if semantic is None:
        semantic = torch.empty(P, dtype=torch.int32, device=cloud.device)
    _lib.run("scene_points_label", label_record(cloud, offset, count, max_blocks, rows, frames, scratch, K, cull,
                                                instance, semantic, points), cloud.device)
    return instance, semantic


def max_blocks_of(count):
    return max(1, -(-int(np.max(count)) // LABEL_BLOCK))


# ---------------------------------------------------------------------------------- the result
class PointLabels(object):
    """label_points' result.  `instance`, `semantic` (P,), `points` (S, cap) int32 and `frames`
    (S, cap, 8) float32 are device tensors (numpy arrays on the host path); `rows` (S,) is the
    detections' count plane.  Indexing, by_name, points_of and save read the host copy, made once."""

    def __init__(self, names, count, offset, cap, prefer, min_score, words, frames):
        self.names, self.count, self.offset, self.cap = list(names), count, offset, int(cap)
        self.prefer, self.min_score, self.frames = prefer, float(min_score), frames
        self._words, self._host = words, None  # rows | points | instance | semantic, one int32 buffer
        self._index = None                     # index()'s PointIndex, built once
        S, P = len(self.names), int(np.sum(count, dtype=np.int64))
        self._cuts = np.cumsum([0, S, S * self.cap, P, P])
        a = self._cuts
        self.rows, self.points = words[a[0]:a[1]], words[a[1]:a[2]].reshape(S, self.cap)
        self.instance, self.semantic = words[a[2]:a[3]], words[a[3]:a[4]]

    def __len__(self):
        return len(self.names)

    def host(self):
        """{rows, points, instance, semantic}: numpy views of the one host copy."""
        if self._host is None:
            w = self._words.cpu().numpy() if torch.is_tensor(self._words) else self._words
            a, S = self._cuts, len(self.names)
            self._host = {"rows": np.clip(w[a[0]:a[1]], 0, self.cap), "points": w[a[1]:a[2]].reshape(S, self.cap),
                          "instance": w[a[2]:a[3]], "semantic": w[a[3]:a[4]]}
        return self._host

    def __getitem__(self, i):
        i = int(i)
        if not -len(self) <= i < len(self):
            raise IndexError(i)
        i %= len(self)
        h, o, n = self.host(), int(self.offset[i]), int(self.count[i])
        return {"instance": h["instance"][o:o + n], "semantic": h["semantic"][o:o + n], "points": h["points"][i]}

    def by_name(self, name):
        return self[self.names.index(name)]

    def index(self):
        """The PointIndex of these labels (votenet/point_index.py): per-row point lists, built once and
        kept; on the device where the labels are device tensors, without a host read, else in numpy."""
        if self._index is None:
            from .point_index import build_index
            self._index = build_index(self.names, self.count, self.offset, self.cap, self.instance)
        return self._index

    def points_of(self, i, row):
        """The indices, in scan i, of the points that packed row `row` owns."""
        if self._index is not None and 0 <= int(row) < self.cap:  # the same array, as a slice of the lists
            return self._index.points_of(i, row).astype(np.int64)
        return np.nonzero(self[i]["instance"] == int(row))[0]

    def save(self, directory, index=False):
        """<name>_labels.npz per scan: instance, semantic, points (cut to the scan's count of
        detections), prefer, min_score; with `index` also the scan's order and start (cut to the scan's
        count of detections plus one) of index()."""
        os.makedirs(directory, exist_ok=True)
        rows = self.host()["rows"]
        lists = self.index() if index else None
        for i, name in enumerate(self.names):
            one = self[i]
            more = {}
            if lists is not None:
                more = {"order": lists[i]["order"], "start": lists[i]["start"][:int(rows[i]) + 1]}
            np.savez(os.path.join(directory, name + "_labels.npz"), instance=one["instance"], semantic=one["semantic"],
                     points=one["points"][:int(rows[i])], prefer=np.array(self.prefer),
                     min_score=np.float64(self.min_score), **more)


def _read_layout(found, S):
    """(cap, NC) of the four planes label_points reads, ValueError where they are not a packed layout."""
    layout = getattr(found, "layout", None)
    if not isinstance(layout, dict) or any(k not in layout for k in ("count", "cls", "score", "box")):
        raise ValueError("label_points: the detections have no count, cls, score and box planes")
    cls, score = tuple(layout["cls"][1]), tuple(layout["score"][1])
    if len(cls) != 2 or cls[0] != S or cls[1] < 1 or tuple(layout["count"][1]) != (S,) or \
            tuple(layout["box"][1]) != cls + (7,) or score[:2] != cls or len(score) > 3:
        raise ValueError("label_points: planes %s do not form (S = %d, cap) rows"
                         % ({k: tuple(layout[k][1]) for k in ("count", "cls", "score", "box")}, S))
    return cls[1], (score[2] if len(score) == 3 else 0)


def label_points(found, store, prefer="score", min_score=0.0, cull=CULL):
    """The owner of every raw row of `store` among the packed detections `found` (module docstring)
    -> PointLabels.  `found`: a Detections or TiledDetections; `store`: a ScanStore whose names equal
    found.names in order.  On the device where the store and the arena share one; else in numpy.
    `cull` does not change the result."""
    _prefer(prefer)
    min_score = _min_score(min_score)
    if not isinstance(found, Detections):
        raise ValueError("label_points: a Detections or a TiledDetections, got %s" % type(found).__name__)
    if not isinstance(store, ScanStore):
        raise ValueError("label_points: a ScanStore, got %s" % type(store).__name__)
    if len(found.names) != len(store.names):
        raise ValueError("label_points: %d scans of detections, %d in the store" % (len(found.names), len(store.names)))
    for i, (a, b) in enumerate(zip(found.names, store.names)):
        if a != b:
            raise ValueError("label_points: scan %d is %r in the detections and %r in the store" % (i, a, b))
    S = len(store.names)
    cap, NC = _read_layout(found, S)
    if found.K < 1 or found.K > MAX_K:
        raise ValueError("label_points: K = %d proposals, 1..%d" % (found.K, MAX_K))
    P = int(np.sum(store.count, dtype=np.int64))
    cuts = np.cumsum([0, S, S * cap, P, P])
    on_device = store.dev is not None and torch.is_tensor(found.arena) and found.arena.device == store.device
    if not on_device:
        planes = found.planes()
        got = host_label_points(planes, store.clouds, prefer, min_score)
        words = np.concatenate([np.asarray(planes["count"], np.int32), got["points"].reshape(-1), got["instance"],
                                got["semantic"]]).astype(np.int32)
        return PointLabels(store.names, store.count, store.offset, cap, prefer, min_score, words, got["frames"])
    arena, d, dev = found.arena, store.dev, store.device
    if arena.dtype != torch.float32 or not arena.is_contiguous():
        raise ValueError("label_points: the arena must be contiguous float32")

    def plane(name, dtype):
        at, shape = found.layout[name]
        flat = arena[at:at + int(np.prod(shape))]
        return (flat if dtype == torch.float32 else flat.view(dtype)).view(*shape)

    count, cls = plane("count", torch.int32), plane("cls", torch.int32)
    words = torch.empty(int(cuts[-1]), dtype=torch.int32, device=dev)
    words[:S].copy_(count)  # device to device: save() cuts `points` by it
    points = words[cuts[1]:cuts[2]].view(S, cap)
    frames, _, scratch = frames_gpu(count, cls, plane("score", torch.float32), plane("box", torch.float32), found.K,
                                    prefer, min_score, points=points)
    label_gpu(d["cloud"], d["offset"], d["count"], max_blocks_of(store.count), count, frames, scratch, found.K, points,
              cull=cull, instance=words[cuts[2]:cuts[3]], semantic=words[cuts[3]:cuts[4]])
    return PointLabels(store.names, store.count, store.offset, cap, prefer, min_score, words, frames)
