"""SUN RGB-D train / eval batches built on the GPU from a resident scene store.

The reference's loaders (sunrgbd/sunrgbd_detection_dataset.py:119-246 and
sunrgbd/sunrgbd_ssl_dataset.py:53-181, :221-312) redo per-scene numpy work in every __getitem__ on
the WHOLE 50k-point scan before they sample it.  Here the preprocessed scans (`<name>_pc.npz`,
`<name>_bbox.npy`, `<name>_votes.npz`, the sunrgbd_pc_bbox_votes_50k_v1_{train,val} folders) are
read ONCE into flat device arrays (`SunRgbdScenes`), and a batch is two kernel launches
(csrc/sunrgbd_batch.hip, include/sunrgbd_hip.h) on the train step's side stream (scene_loader.feed).

The vote rows are a pure function of the cloud and the boxes (the vote loop of the reference's
extraction, sunrgbd/sunrgbd_data.py:232-257).  `votes="boxes"` loads a folder that holds only
`_pc.npz` and `_bbox.npy`: the store then keeps no vote rows and the batch builder computes them per
sampled point (`compute_votes` is the numpy restatement; `SunRgbdScenes.vote_rows` and
`export_votes` give the whole store's rows, the latter in the reference's file layout).
`SunRgbdScenes.from_raw` builds such a store straight from a raw `sunrgbd_trainval/` folder
(votenet/sunrgbd_raw.py) and `export` writes its `_pc.npz` / `_bbox.npy`.

What differs from the ScanNet loader: boxes are oriented (heading class / residual of 12 bins, size
residuals from 2 x the stored half sizes), the vote labels are carried through the augmentation
(read from `_votes.npz` by default, computed from the boxes with votes="boxes"), the labeled and the unlabeled dataset normalise colour differently (rgb - 0.5 and
(rgb - 0.5) / 256: the store keeps the first, the second is applied per row at build time), and the
detection dataset augments colour per point.  Only that is here: the draw hash, the sampler, the
store's and the loader's skeleton, the launch, epoch_plan, feed and eval_batches are scene_loader's,
shared with scannet_data and scan_data and re-exported here.

Keys, dtypes and shapes are those of data.make_batch (pretrain, eval) and data.make_semi_batch
(semi-supervised) for sunrgbd_config(); semi batches also carry `supervised_mask_host`.
"""
import importlib
import os

import numpy as np
import torch

from .. import records
from . import sunrgbd_raw as raw
from .scene_loader import (DRAW_EMA, DRAW_STUDENT, MAX_BATCH, MAX_NUM_OBJ, SceneError, SceneLoader,  # noqa: F401
                           SceneStore, _element, _read_list, draw_key, epoch_plan, eval_batches, feed,
                           launch, rotz, sample_indices, unit_uniform)

NUM_CLASS = 10     # model_util_sunrgbd.py:21
MEAN_COLOR_RGB = np.array([0.5, 0.5, 0.5])  # sunrgbd_detection_dataset.py:41 (colour is in 0~1)
VOTE_COLS = 10     # mask, three votes
# draw indices of the hash beyond the two point samples (sunrgbd_hip.h)
DRAW_FLIP, DRAW_ANGLE, DRAW_SCALE, DRAW_COLOR, DRAW_JITTER, DRAW_DROP = 2, 3, 4, 5, 11, 12


# ------------------------------------------------------------------ reading scans and splits
def _votes_mode(votes):
    if votes not in ("file", "boxes"):
        raise ValueError("votes must be 'file' or 'boxes', got %r" % (votes,))
    return votes


def read_scene(data_dir, name, use_color=False, use_height=True, votes="file"):
    """One preprocessed scan -> the per-scene state the batches are built from, computed once in the
    file's dtype as the reference does and then held in float32: cloud (n, C) = xyz, [rgb - 0.5],
    [z - floor]; the floor height (np.percentile(z, 0.99)); the vote rows (n, 10) float32; the box
    table (K, 8) float64 = centre, half sizes, heading, class.  votes="boxes": `_votes.npz` is
    neither required nor opened and the scene's "votes" is None (compute_votes gives the rows)."""
    from_file = _votes_mode(votes) == "file"
    paths = {"pc": os.path.join(data_dir, name + "_pc.npz"), "bbox": os.path.join(data_dir, name + "_bbox.npy")}
    if from_file:
        paths["votes"] = os.path.join(data_dir, name + "_votes.npz")
    for p in paths.values():
        if not os.path.exists(p):
            raise SceneError("scan %s: missing %s" % (name, p))
    with np.load(paths["pc"]) as f:
        if "pc" not in f.files:
            raise SceneError("scan %s: %s has no 'pc'" % (name, paths["pc"]))
        pc = f["pc"]
    votes = None
    if from_file:
        with np.load(paths["votes"]) as f:
            if "point_votes" not in f.files:
                raise SceneError("scan %s: %s has no 'point_votes'" % (name, paths["votes"]))
            votes = f["point_votes"]
    bbox = np.load(paths["bbox"])
    if pc.ndim != 2 or pc.shape[1] < (6 if use_color else 3):
        raise SceneError("scan %s: pc has shape %s, expected (n, %s)"
                         % (name, pc.shape, ">= 6" if use_color else ">= 3"))
    n = pc.shape[0]
    if n == 0 or n >= 1 << 30:
        raise SceneError("scan %s: %d points" % (name, n))
    if from_file and (votes.ndim != 2 or votes.shape[0] != n or votes.shape[1] != VOTE_COLS):
        raise SceneError("scan %s: %d points but point_votes has shape %s, expected (%d, %d)"
                         % (name, n, votes.shape, n, VOTE_COLS))
    if bbox.size == 0:
        bbox = np.zeros((0, 8))
    elif bbox.ndim != 2 or bbox.shape[1] != 8:
        raise SceneError("scan %s: _bbox.npy has shape %s, expected (boxes, 8)" % (name, bbox.shape))
    if bbox.shape[0] > MAX_NUM_OBJ:
        raise SceneError("scan %s: %d boxes, at most MAX_NUM_OBJ = %d" % (name, bbox.shape[0], MAX_NUM_OBJ))
    for i, label in enumerate(bbox[:, 7]):
        if not (0 <= label < NUM_CLASS and label == int(label)):
            raise SceneError("scan %s: box %d has class %g, not one of 0..%d"
                             % (name, i, float(label), NUM_CLASS - 1))
    if pc.dtype not in (np.float32, np.float64):
        pc = pc.astype(np.float64)
    if use_color:
        cloud = np.array(pc[:, 0:6])
        cloud[:, 3:] = cloud[:, 3:] - MEAN_COLOR_RGB
    else:
        cloud = np.array(pc[:, 0:3])
    floor = np.percentile(cloud[:, 2], 0.99)
    if use_height:
        cloud = np.concatenate([cloud, np.expand_dims(cloud[:, 2] - floor, 1)], 1)
    return {"name": name, "cloud": np.ascontiguousarray(cloud, np.float32), "floor": float(floor),
            "votes": np.ascontiguousarray(votes, np.float32) if from_file else None,
            "boxes": np.array(bbox, np.float64), "dtype": str(pc.dtype)}


def compute_votes(cloud_xyz, boxes):
    """The vote rows (n, 10) float32 of the points `cloud_xyz` (n, >= 3; the store's float32 cloud)
    from the box table `boxes` (K, 8), by the rule of the reference's extraction
    (sunrgbd/sunrgbd_data.py:232-257; the hull of sunrgbd_utils.py:227-237 is the oriented box): in
    float64, d = p - centre, lx = d.x cos t - d.y sin t, ly = d.x sin t + d.y cos t, inside iff
    |lx| <= |l|, |ly| <= |w|, |d.z| <= |h|.  In table order the first containing box sets the mask
    and all three votes to float32(centre - p), the second the second vote, the third and every later
    one the third (the LAST containing box stays there).  A box with a zero half size contains nothing
    (the reference's hull call raises on its flat corners and the object is skipped).  This is
    csrc/sunrgbd_batch.hip:sun_vote_row."""
    p = np.asarray(cloud_xyz)[:, 0:3].astype(np.float64)
    boxes = np.asarray(boxes, np.float64).reshape(-1, 8)
    rows = np.zeros((p.shape[0], VOTE_COLS), np.float32)
    hits = np.zeros(p.shape[0], np.int64)
    for k in range(boxes.shape[0]):
        half = np.abs(boxes[k, 3:6])
        if (half == 0).any():
            continue
        d = p - boxes[k, 0:3]
        c, s = np.cos(boxes[k, 6]), np.sin(boxes[k, 6])
        lx, ly = d[:, 0] * c - d[:, 1] * s, d[:, 0] * s + d[:, 1] * c
        within = (np.abs(lx) <= half[0]) & (np.abs(ly) <= half[1]) & (np.abs(d[:, 2]) <= half[2])
        v = (boxes[k, 0:3] - p).astype(np.float32)
        first, second, later = within & (hits == 0), within & (hits == 1), within & (hits >= 2)
        rows[first, 0] = 1.0
        rows[first, 1:10] = np.tile(v[first], (1, 3))
        rows[second, 4:7] = v[second]
        rows[later, 7:10] = v[later]
        hits += within
    return rows


def available_scans(data_dir):
    """The scan names of a folder: the first six characters of its file names
    (sunrgbd_detection_dataset.py:58-59)."""
    return sorted(set(os.path.basename(f)[0:6] for f in os.listdir(data_dir)))


def labeled_split(data_dir, list_path):
    """The labeled scans of a list file such as sunrgbd_v1_train_0.05.txt
    (sunrgbd_ssl_dataset.py:37-40); listed scans without files are skipped."""
    avail = set(available_scans(data_dir))
    return [s for s in _read_list(list_path) if s in avail]


def unlabeled_split(data_dir, list_path):
    """train minus labeled, or all of train when the two have equal length
    (sunrgbd_ssl_dataset.py:193-203); sorted."""
    train = available_scans(data_dir)
    labeled = _read_list(list_path)
    names = list(train) if len(train) == len(labeled) else list(set(train) - set(labeled))
    return sorted(names)


def val_split(val_dir):
    """Every scan of the val folder (sunrgbd_detection_dataset.py:51-59)."""
    return available_scans(val_dir)


# ------------------------------------------------------------------ the resident store
class SunRgbdScenes(SceneStore):
    """Every scan of `scan_names` read once and packed into flat device arrays with a per-scene
    offset / count table: the cloud (P, C) float32, the vote rows (P, 10) float32, the box table
    (S, 64, 8) float64.  At 50k points a scene is 50k x (4 C + 40) bytes = 2.8 MB with the height
    channel, 4 MB with colour too.  votes="boxes": no `_votes.npz` is read and no vote rows are
    kept (50k x 4 C bytes a scene: 0.8 MB, 1.4 MB with colour); the batch builder computes them from
    the boxes.  `device=None` keeps the host copy only (the CPU path)."""

    def __init__(self, data_dir, scan_names, device, use_color=False, use_height=True, votes="file"):
        self.votes = _votes_mode(votes)
        self.use_color, self.use_height = use_color, use_height
        SceneStore.__init__(self, data_dir, scan_names,
                            lambda s: read_scene(data_dir, s, use_color, use_height, votes), device, box_cols=8)
        self.floor = np.array([s["floor"] for s in self.scenes], np.float64)
        if self.dev is not None and self.votes == "file":
            self.dev["votes"] = self._flat("votes")
        self.raw_export = None

    @classmethod
    def from_raw(cls, trainval_dir, scenes, device, use_color=False, use_height=True, use_v1=True,
                 num_point=raw.NUM_POINT, seed=0, choices=None):
        """The votes="boxes" store of SunRgbdScenes(exported_dir, ...) straight from a raw
        `sunrgbd_trainval/` folder (`depth/%06d.mat`, `label_v1/%06d.txt` or, without use_v1,
        `label/%06d.txt`): sunrgbd_raw.export_trainval on `device` (None: its numpy restatement), a
        chunk of raw clouds in host memory at a time; nothing is written.  `scenes`: data indices or
        their six-digit names, or the path of an index list such as train_data_idx.txt.  Scene number
        i keeps `choices[name]` or the draw (seed, 0, i).  The kept rows and the box tables stay on
        the host for `export`."""
        names = raw.read_idx_list(scenes) if isinstance(scenes, str) else [raw.scene_name(s) for s in scenes]
        if not names:
            raise SceneError("no scans to load from %s" % trainval_dir)
        records = (raw.read_trainval_scene(trainval_dir, s, use_v1) for s in names)
        exported = dict(zip(names, raw.export_trainval(records, device, num_point, seed, choices)))
        cols = [0, 1, 2] + ([3, 4, 5] if use_color else []) + ([6] if use_height else [])

        def read(s):
            e = exported[s]
            return {"name": s, "cloud": np.ascontiguousarray(e["rows"][:, cols]), "floor": float(e["floor"]),
                    "votes": None, "boxes": e["bbox"], "dtype": str(e["pc"].dtype)}

        self = cls.__new__(cls)
        self.votes, self.use_color, self.use_height = "boxes", use_color, use_height
        SceneStore.__init__(self, trainval_dir, names, read, device, box_cols=8)
        self.floor = np.array([s["floor"] for s in self.scenes], np.float64)
        self.raw_export = {s: {"pc": e["pc"], "bbox": e["bbox"]} for s, e in exported.items()}
        return self

    def export(self, out_dir):
        """Write `<name>_pc.npz` and `<name>_bbox.npy` of every scene of a from_raw store; with
        export_votes(out_dir) the folder loads in the reference and as a "file" store."""
        if self.raw_export is None:
            raise RuntimeError("SunRgbdScenes.export: only a from_raw store holds the arrays to write")
        os.makedirs(out_dir, exist_ok=True)
        for s in self.scan_names:
            raw.save_export(out_dir, s, self.raw_export[s])

    def vote_rows(self):
        """The (P, 10) float32 vote rows of the whole store on the device, in the reference's layout
        (mask, three votes): the stored rows of a "file" store, one scene_sunrgbd_votes launch on the
        current stream for a "boxes" store."""
        if self.dev is None:
            raise RuntimeError("SunRgbdScenes: the store has no device copy (device=None); use compute_votes")
        if self.votes == "file":
            return self.dev["votes"]
        _L = importlib.import_module("3dioumatch_amd._lib")
        d = self.dev
        out = torch.empty((d["cloud"].shape[0], VOTE_COLS), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _L.check(_L.lib.scene_sunrgbd_votes(d["cloud"].data_ptr(), self.channels, d["offset"].data_ptr(),
                                                d["count"].data_ptr(), d["boxes"].data_ptr(),
                                                d["nbox"].data_ptr(), len(self.scenes), out.data_ptr(),
                                                torch.cuda.current_stream(self.device).cuda_stream),
                     "scene_sunrgbd_votes")
        return out

    def export_votes(self, out_dir):
        """Write `<name>_votes.npz` with 'point_votes' (n, 10) float64 for every scan: the layout of
        the reference's extraction (sunrgbd/sunrgbd_data.py:260-261), so that a folder prepared here
        loads in the reference and as a "file" store.  The rows are vote_rows()'s (compute_votes'
        for a store without a device copy)."""
        if self.dev is not None:
            rows = self.vote_rows().cpu().numpy()
        else:
            rows = np.concatenate([s["votes"] if s["votes"] is not None else
                                   compute_votes(s["cloud"], s["boxes"]) for s in self.scenes])
        os.makedirs(out_dir, exist_ok=True)
        for name, off, n in zip(self.scan_names, self.offset, self.count):
            np.savez_compressed(os.path.join(out_dir, name + "_votes.npz"),
                                point_votes=rows[off:off + n].astype(np.float64))


# ------------------------------------------------------------------ host restatement
def augmentation(u):
    """uniforms -> (flip_x, angle, scale) with the reference's formulas
    (sunrgbd_detection_dataset.py:155-191)."""
    return int(u[0] > 0.5), (u[1] * np.pi / 3) - np.pi / 6, u[2] * 0.3 + 0.85


def angle2class(angle, num_heading_bin):
    """model_util_sunrgbd.py:92-108 (float64, Python's float modulo)."""
    angle = angle % (2 * np.pi)
    per = 2 * np.pi / float(num_heading_bin)
    shifted = (angle + per / 2) % (2 * np.pi)
    class_id = int(shifted / per)
    return class_id, shifted - (class_id * per + per / 2)


def host_scene(scene, idx, u=None, votes=True, boxes="raw", mean_size=None, has_height=True,
               num_heading_bin=12, div256=False, color=None):
    """One scene of a batch in numpy, in the reference's arithmetic: the sample `idx`, the
    augmentation of the uniforms `u` (None: none), the colour augmentation `color` = (u_color (6,),
    u_jitter (n,), u_drop (n,)) by source point, vote labels, box labels ('aug': in the augmented
    frame, 'raw': un-augmented, None: none).  Every per-point operation of the reference commutes
    with the sampling, so only the sampled rows are computed."""
    idx = np.asarray(idx)
    pc = scene["cloud"][idx].copy()
    has_color = pc.shape[1] >= 6
    if div256 and has_color:
        pc[:, 3:6] = pc[:, 3:6] / 256.0
    bb = scene["boxes"].copy()
    out = {}
    pv = None
    if votes:  # a scene without vote rows: from the boxes (the rule is per point: only the sample)
        pv = scene["votes"][idx] if scene["votes"] is not None else compute_votes(scene["cloud"][idx], bb)
        pv = pv.astype(np.float64)
    if u is not None:
        fx, angle, scale = augmentation(u)
        aug_boxes = boxes == "aug"
        if fx:
            pc[:, 0] = -1 * pc[:, 0]
            if aug_boxes:
                bb[:, 0] = -1 * bb[:, 0]
                bb[:, 6] = np.pi - bb[:, 6]
            if votes:
                pv[:, [1, 4, 7]] = -1 * pv[:, [1, 4, 7]]
        rot = rotz(angle)
        pc[:, 0:3] = np.dot(pc[:, 0:3], np.transpose(rot))
        if aug_boxes:
            bb[:, 0:3] = np.dot(bb[:, 0:3], np.transpose(rot))
            bb[:, 6] -= angle
        c, s = rot[0, 0], rot[1, 0]
        if votes:  # rot(p + v) - rot(p) as rot(v), elementwise in the device's order
            for k in (1, 4, 7):
                x, y, z = pv[:, k].copy(), pv[:, k + 1].copy(), pv[:, k + 2].copy()
                pv[:, k] = x * c + y * -s + z * 0.0
                pv[:, k + 1] = x * s + y * c + z * 0.0
                pv[:, k + 2] = x * 0.0 + y * 0.0 + z * 1.0
        if color is not None and has_color:
            u_color, u_jit, u_drop = color
            rgb = pc[:, 3:6] + MEAN_COLOR_RGB
            rgb *= (1 + 0.4 * np.asarray(u_color[0:3]) - 0.2)
            rgb += (0.1 * np.asarray(u_color[3:6]) - 0.05)
            rgb += np.expand_dims((0.05 * np.asarray(u_jit)[idx] - 0.025), -1)
            rgb = np.clip(rgb, 0, 1)
            rgb *= np.expand_dims(np.asarray(u_drop)[idx] > 0.3, -1)
            pc[:, 3:6] = rgb - MEAN_COLOR_RGB
        scale_ratio = np.expand_dims(np.tile(scale, 3), 0)
        pc[:, 0:3] *= scale_ratio
        if aug_boxes:
            bb[:, 0:3] *= scale_ratio
            bb[:, 3:6] *= scale_ratio
        if votes:
            for k in (1, 4, 7):
                pv[:, k:k + 3] *= scale_ratio
        if has_height:
            pc[:, -1] *= scale_ratio[0, 0]
        out.update(flip_x_axis=fx, flip_y_axis=0, rot_mat=rot.astype(np.float32),
                   rot_angle=np.float32(angle), scale=scale_ratio.astype(np.float32))
    else:
        out.update(flip_x_axis=0, flip_y_axis=0, rot_mat=np.identity(3, np.float32),
                   rot_angle=np.float32(0), scale=np.ones((1, 3), np.float32))
    out["point_clouds"] = pc.astype(np.float32)
    if votes:
        out["vote_label"] = pv[:, 1:].astype(np.float32)
        out["vote_label_mask"] = pv[:, 0].astype(np.int64)
    if boxes is not None:
        nb = bb.shape[0]
        target = np.zeros((MAX_NUM_OBJ, 6))
        target[:nb] = bb[:, 0:6]
        angle_classes, angle_residuals = np.zeros(MAX_NUM_OBJ), np.zeros(MAX_NUM_OBJ)
        size_classes, size_residuals = np.zeros(MAX_NUM_OBJ), np.zeros((MAX_NUM_OBJ, 3))
        mask = np.zeros(MAX_NUM_OBJ, np.float32)
        mask[:nb] = 1
        for i in range(nb):
            cls = int(bb[i, 7])
            angle_classes[i], angle_residuals[i] = angle2class(bb[i, 6], num_heading_bin)
            size_classes[i] = cls
            size_residuals[i] = bb[i, 3:6] * 2 - mean_size[cls]
        out.update(center_label=target.astype(np.float32)[:, 0:3],
                   heading_class_label=angle_classes.astype(np.int64),
                   heading_residual_label=angle_residuals.astype(np.float32),
                   size_class_label=size_classes.astype(np.int64),
                   size_residual_label=size_residuals.astype(np.float32),
                   sem_cls_label=size_classes.astype(np.int64), box_label_mask=mask)
    return out


def uniforms(seed, counter, row):
    """The three uniforms in [0, 1) of a row: flip, angle, scale (float64, 32 bits)."""
    return unit_uniform(draw_key(seed, counter, row, DRAW_FLIP + np.arange(3)))


def color_uniforms(seed, counter, row):
    """The six colour uniforms of a row: brightness rgb, shift rgb."""
    return unit_uniform(draw_key(seed, counter, row, DRAW_COLOR + np.arange(6)))


def point_uniforms(seed, counter, row, n):
    """(2, n): the jitter and the drop uniform of every SOURCE point of a row's scene."""
    p = np.arange(n, dtype=np.uint32)
    return np.stack([unit_uniform(_element(draw_key(seed, counter, row, d), p)) for d in (DRAW_JITTER, DRAW_DROP)])


# ------------------------------------------------------------------ batches
class SunRgbdLoader(SceneLoader):
    """SceneLoader with the semantics of the reference's SUN RGB-D datasets:

      pretrain_batch   SunrgbdDetectionVotesDataset('train', augment=True), with its per-point colour
                       augmentation when the store has colour
      semi_batch       SunrgbdSSLLabeledDataset + SunrgbdSSLUnlabeledDataset rows (augment=True)
      eval_batch       SunrgbdDetectionVotesDataset('val', augment=False)

    `config`: sunrgbd_config(mean_size_arr=...).  Per-point colour draws are keyed additionally by
    the source point index.  Explicit draws: {'idx': (B, N) ints, 'ema_idx': (B, N), 'u': (B, 3)
    float64 uniforms (flip, angle, scale), 'u_color': (B, 6), 'u_point': (B, 2, n_max) jitter and
    drop by source point}."""
    _Args, _ENTRY, _DATASET = records.SunBatchArgs, "scene_sunrgbd_batch_build", "sunrgbd"
    _STORE_KEYS = ("cloud", "offset", "count", "boxes", "nbox")
    _UNIFORMS = {"u": 3, "u_color": 6}
    _uniforms = staticmethod(uniforms)

    def _color_aug(self, kind):
        return kind == "pretrain" and self.scenes.use_color

    def _given(self, draws, counts):
        given = SceneLoader._given(self, draws, counts)
        if "u_point" in draws:
            v = np.asarray(draws["u_point"], np.float64)
            B, n_max = len(counts), int(counts.max())
            if v.ndim != 3 or v.shape[0] != B or v.shape[1] != 2 or v.shape[2] < n_max:
                raise ValueError("explicit draws 'u_point' have shape %s, expected (%d, 2, >= %d)"
                                 % (v.shape, B, n_max))
            given["u_point"] = np.ascontiguousarray(v)
        return given

    def _fill(self, a, kind, nl, given, scratch):
        a.color_aug = int(self._color_aug(kind))
        a.div256_from = nl if kind == "semi" else a.B
        a.num_heading_bin = int(self.config.num_heading_bin)
        d = self.scenes.dev
        a.votes = d["votes"].data_ptr() if "votes" in d else None  # NULL: computed from the boxes
        if "u_point" in given:
            a.u_point_stride = given["u_point"].shape[2]

    def _extra_host_draws(self, draws, kind, counter, n):
        if self._color_aug(kind):
            B = len(n)
            draws["u_color"] = np.stack([color_uniforms(self.seed, counter, r) for r in range(B)])
            up = np.zeros((B, 2, int(n.max())))
            for r in range(B):
                up[r, :, :n[r]] = point_uniforms(self.seed, counter, r, n[r])
            draws["u_point"] = up

    def _host_row(self, scene, kind, r, labeled, idx, u, boxes, draws):
        color = None
        if self._color_aug(kind):
            up = np.asarray(draws["u_point"])[r]
            color = (np.asarray(draws["u_color"])[r], up[0], up[1])
        return host_scene(scene, idx, u, votes=labeled, boxes=boxes, mean_size=self.mean_size,
                          has_height=self.scenes.use_height, num_heading_bin=self.config.num_heading_bin,
                          div256=kind == "semi" and not labeled, color=color)

    def _teacher_colour(self, ema, labeled):
        if not labeled and self.scenes.use_color:  # the unlabeled dataset's (rgb - 0.5) / 256
            ema[:, 3:6] = ema[:, 3:6] / 256.0
        return ema


# ------------------------------------------------------------------ synthetic scans
def write_synthetic_scans(data_dir, names, num_points=50000, boxes=12, seed=0, dtype=np.float32):
    """Seeded SUN RGB-D-sized stand-ins in the on-disk layout (for tests and tools/, where no dataset
    is at hand): `boxes` oriented boxes, some of them overlapping; two thirds of the points fall
    inside a box; a point's vote row holds the offsets to the centres of the first three boxes that
    contain it (one box: the vote three times; two: first, second, first), mask 1."""
    g = np.random.default_rng(seed)
    for name in names:
        box = np.zeros((boxes, 8))
        box[:, 0:3] = g.random((boxes, 3)) * [5.0, 4.0, 1.5] + [-2.5, 1.0, -1.0]
        if boxes > 2:  # overlapping boxes: points with two and three votes
            box[1, 0:3] = box[0, 0:3] + [0.1, -0.1, 0.05]
            box[2, 0:3] = box[0, 0:3] + [-0.1, 0.05, 0.0]
        box[:, 3:6] = g.random((boxes, 3)) * 0.6 + 0.15
        box[:, 6] = g.random(boxes) * 2 * np.pi - np.pi
        box[:, 7] = g.integers(0, NUM_CLASS, boxes)
        xyz = g.random((num_points, 3)) * [6.0, 5.0, 2.5] + [-3.0, 0.5, -1.3]
        if boxes:
            inside = np.where(g.random(num_points) < 2.0 / 3.0)[0]
            b = g.integers(0, boxes, inside.size)
            local = (g.random((inside.size, 3)) * 2 - 1) * box[b, 3:6]
            c, s = np.cos(box[b, 6]), np.sin(box[b, 6])
            xyz[inside, 0] = box[b, 0] + local[:, 0] * c + local[:, 1] * s
            xyz[inside, 1] = box[b, 1] - local[:, 0] * s + local[:, 1] * c
            xyz[inside, 2] = box[b, 2] + local[:, 2]
        xyz = xyz.astype(dtype)
        votes = np.zeros((num_points, VOTE_COLS))
        hits = np.zeros(num_points, np.int64)
        for k in range(boxes):
            d = xyz.astype(np.float64) - box[k, 0:3]
            c, s = np.cos(box[k, 6]), np.sin(box[k, 6])
            lx, ly = d[:, 0] * c - d[:, 1] * s, d[:, 0] * s + d[:, 1] * c
            within = (np.abs(lx) <= box[k, 3] + 1e-9) & (np.abs(ly) <= box[k, 4] + 1e-9) & \
                (np.abs(d[:, 2]) <= box[k, 5] + 1e-9)
            first, second, third = within & (hits == 0), within & (hits == 1), within & (hits == 2)
            votes[first, 0] = 1.0
            votes[first, 1:10] = np.tile(-d[first], (1, 3))
            votes[second, 4:7] = -d[second]
            votes[third, 7:10] = -d[third]
            hits += within
        rgb = g.random((num_points, 3)).astype(dtype)
        np.savez(os.path.join(data_dir, name + "_pc.npz"), pc=np.concatenate([xyz, rgb], 1))
        np.save(os.path.join(data_dir, name + "_bbox.npy"), box)
        np.savez(os.path.join(data_dir, name + "_votes.npz"), point_votes=votes)
