"""ScanNet train / eval batches built on the GPU from a resident scene store.

The reference's loaders (scannet/scannet_ssl_dataset.py:47-184, :224-320 and
scannet/scannet_detection_dataset.py:85-223) redo per-scene numpy work in every __getitem__: two
random subsets, flip / rotate / scale, a Python loop over the instances for the vote labels.
Here the preprocessed scans (`<scan>_vert.npy`, `_ins_label.npy`, `_sem_label.npy`, `_bbox.npy`,
as batch_load_scannet_data.py writes them) are read ONCE into flat device arrays
(`ScanNetScenes`), and a batch is three kernel launches (csrc/scene_batch.hip, include/scene_hip.h)
on the train step's side stream (`feed`), so no step waits on the host.

Every random draw is a counter-based hash of (seed, batch counter, batch row, draw index); a batch
is a pure function of its arguments.  `host_*` restate the whole construction in numpy -- the same
hash, the same bijection, the reference's own float64 / float32 arithmetic -- which is the CPU path
and the yardstick of the device path.

What this module holds is ScanNet's own: the reader, the splits, the augmentation, host_scene, the
args record.  The hash, the sampler, the store's and the loader's skeleton, the launch, epoch_plan,
feed and eval_batches are scene_loader's, shared with sunrgbd_data and scan_data and re-exported here.

Keys, dtypes and shapes are those of data.make_batch (pretrain, eval) and data.make_semi_batch
(semi-supervised); semi batches also carry `supervised_mask_host`.
"""
import os

import numpy as np
import torch

from .. import records
from . import scannet_raw as raw
from .scene_loader import (DRAW_EMA, DRAW_STUDENT, MAX_BATCH, MAX_NUM_OBJ, SceneError, SceneLoader,  # noqa: F401
                           SceneStore, _read_list, draw_key, epoch_plan, eval_batches, feed, launch,
                           rotz, sample_indices, unit_uniform)

MAX_INSTANCES = 1024  # dense instance ids per scene (SB_MAX_INST)
MEAN_COLOR_RGB = np.array([109.8, 97.2, 83.8])  # scannet_ssl_dataset.py:21
NYU40IDS = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39])  # model_util_scannet.py:30
DRAW_UNIFORM = 2  # draw index of the first of a row's four uniforms (scene_hip.h)


def uniforms(seed, counter, row):
    """The four uniforms in [0, 1) of a row: flip x, flip y, angle, scale (float64, 32 bits)."""
    return unit_uniform(draw_key(seed, counter, row, DRAW_UNIFORM + np.arange(4)))


def augmentation(u):
    """uniforms -> (flip_x, flip_y, angle, scale) with the reference's formulas
    (scannet_ssl_dataset.py:102-124)."""
    return (int(u[0] > 0.5), int(u[1] > 0.5), (u[2] * np.pi / 18) - np.pi / 36, u[3] * 0.3 + 0.85)


def rotate_aligned_boxes(input_boxes, rot_mat):  # model_util_scannet.py:85-106
    centers, lengths = input_boxes[:, 0:3], input_boxes[:, 3:6]
    new_centers = np.dot(centers, np.transpose(rot_mat))
    dx, dy = lengths[:, 0] / 2.0, lengths[:, 1] / 2.0
    new_x = np.zeros((dx.shape[0], 4))
    new_y = np.zeros((dx.shape[0], 4))
    for i, crnr in enumerate([(-1, -1), (1, -1), (1, 1), (-1, 1)]):
        crnrs = np.zeros((dx.shape[0], 3))
        crnrs[:, 0] = crnr[0] * dx
        crnrs[:, 1] = crnr[1] * dy
        crnrs = np.dot(crnrs, np.transpose(rot_mat))
        new_x[:, i] = crnrs[:, 0]
        new_y[:, i] = crnrs[:, 1]
    new_lengths = np.stack((2.0 * np.max(new_x, 1), 2.0 * np.max(new_y, 1), lengths[:, 2]), axis=1)
    return np.concatenate([new_centers, new_lengths], axis=1)


# ------------------------------------------------------------------ reading scans and splits
def read_scene(data_dir, name, use_color=False, use_height=True):
    """One preprocessed scan -> the per-scene state the batches are built from, computed once:
    cloud (n, C) float32 = xyz, [(rgb - MEAN_COLOR_RGB) / 256], [z - floor]; the floor height
    (np.percentile(z, 0.99) of the raw cloud, as every __getitem__ of the reference recomputes it);
    dense instance ids; semantic ids; the box table (nb, 7) float64 = centre, size, class index."""
    paths = {k: os.path.join(data_dir, name + "_%s.npy" % k) for k in ("vert", "ins_label", "sem_label", "bbox")}
    for k, p in paths.items():
        if not os.path.exists(p):
            raise SceneError("scan %s: missing %s" % (name, p))
    return scene_from_arrays(name, np.load(paths["vert"]), np.load(paths["ins_label"]),
                             np.load(paths["sem_label"]), np.load(paths["bbox"]), use_color, use_height)


def scene_from_arrays(name, vert, ins, sem, bbox, use_color=False, use_height=True):
    """read_scene's scene from the four arrays themselves, as the files hold them or as
    scannet_raw.export_raw_scans returns them."""
    ins, sem = np.asarray(ins).reshape(-1), np.asarray(sem).reshape(-1)
    n = vert.shape[0] if vert.ndim else 0
    if vert.ndim != 2 or vert.shape[1] < (6 if use_color else 3):
        raise SceneError("scan %s: _vert.npy has shape %s, expected (n, %s)"
                         % (name, vert.shape, "6" if use_color else ">= 3"))
    if n == 0 or n >= 1 << 30:
        raise SceneError("scan %s: %d points" % (name, n))
    if ins.shape[0] != n or sem.shape[0] != n:
        raise SceneError("scan %s: %d vertices but %d instance and %d semantic labels"
                         % (name, n, ins.shape[0], sem.shape[0]))
    if bbox.size == 0:
        bbox = np.zeros((0, 7))
    elif bbox.ndim != 2 or bbox.shape[1] != 7:
        raise SceneError("scan %s: _bbox.npy has shape %s, expected (boxes, 7)" % (name, bbox.shape))
    if bbox.shape[0] > MAX_NUM_OBJ:
        raise SceneError("scan %s: %d boxes, at most MAX_NUM_OBJ = %d" % (name, bbox.shape[0], MAX_NUM_OBJ))
    cls = np.zeros(bbox.shape[0], np.int64)
    for i, label in enumerate(bbox[:, -1]):
        hit = np.where(NYU40IDS == label)[0]
        if hit.size == 0:
            raise SceneError("scan %s: box %d has label %g, not one of the 18 nyu40ids %s"
                             % (name, i, float(label), NYU40IDS.tolist()))
        cls[i] = hit[0]
    ids, dense = np.unique(ins, return_inverse=True)
    if ids.size > MAX_INSTANCES:
        raise SceneError("scan %s: %d instance ids, at most %d" % (name, ids.size, MAX_INSTANCES))
    vert = vert.astype(np.float32, copy=False)
    if use_color:
        cloud = np.array(vert[:, 0:6])
        cloud[:, 3:] = (cloud[:, 3:] - MEAN_COLOR_RGB) / 256.0
    else:
        cloud = np.array(vert[:, 0:3])
    floor = np.percentile(cloud[:, 2], 0.99)
    if use_height:
        cloud = np.concatenate([cloud, np.expand_dims(cloud[:, 2] - floor, 1)], 1)
    boxes = np.zeros((bbox.shape[0], 7))
    boxes[:, 0:6] = bbox[:, 0:6]
    boxes[:, 6] = cls
    return {"name": name, "cloud": np.ascontiguousarray(cloud, np.float32), "floor": floor,
            "inst": dense.astype(np.int32).reshape(-1), "ninst": int(ids.size),
            "sem": sem.astype(np.int32), "boxes": boxes}



def available_scans(data_dir):
    return sorted(set(f[:12] for f in os.listdir(data_dir) if f.startswith("scene")))


def _have(data_dir, names):
    avail = set(available_scans(data_dir))
    return [s for s in names if s in avail]


def labeled_split(data_dir, meta_dir, labeled_list):
    """The labeled scans (scannet_ssl_dataset.py:29-31), e.g. labeled_list='scannetv2_train_0.1.txt';
    listed scans without files are skipped."""
    return _have(data_dir, _read_list(os.path.join(meta_dir, labeled_list)))


def unlabeled_split(data_dir, meta_dir, labeled_list):
    """train minus labeled, sorted (scannet_ssl_dataset.py:192-211)."""
    train = _have(data_dir, _read_list(os.path.join(meta_dir, "scannetv2_train.txt")))
    labeled = _read_list(os.path.join(meta_dir, labeled_list))
    names = list(train) if len(train) == len(labeled) else list(set(train) - set(labeled))
    return sorted(names)


def val_split(data_dir, meta_dir):
    """scannetv2_val.txt (scannet_detection_dataset.py:41-50)."""
    return _have(data_dir, _read_list(os.path.join(meta_dir, "scannetv2_val.txt")))


# ------------------------------------------------------------------ the resident store
class ScanNetScenes(SceneStore):
    """Every scan of `scan_names` read once and packed into flat device arrays with a per-scene
    offset / count table (the whole ScanNet train split is ~1.5 GB at <= 50k points per scan).
    `device=None` keeps the host copy only (the CPU path)."""

    def __init__(self, data_dir, scan_names, device, use_color=False, use_height=True):
        self._pack(data_dir, scan_names, lambda s: read_scene(data_dir, s, use_color, use_height), device,
                   use_color, use_height)

    def _pack(self, data_dir, scan_names, read, device, use_color, use_height):
        self.use_color, self.use_height = use_color, use_height
        self.raw_export = None
        SceneStore.__init__(self, data_dir, scan_names, read, device, box_cols=7)
        self.ninst = np.array([s["ninst"] for s in self.scenes], np.int32)
        self.floor = np.array([s["floor"] for s in self.scenes], np.float32)
        if self.dev is not None:
            self.dev.update(inst=self._flat("inst"), sem=self._flat("sem"), ninst=self._upload(self.ninst))

    @classmethod
    def from_raw(cls, raw_dir, scan_names, label_map, device, use_color=False, use_height=True,
                 max_points=50000, seed=0):
        """The store of ScanNetScenes(exported_dir, ...) straight from raw scan folders
        (`raw_dir/<scan>/<scan>_vh_clean_2.ply`, `.aggregation.json`, `_vh_clean_2.0.010000.segs.json`,
        `.txt`): scannet_raw.export_raw_scans on `device` (None: its numpy restatement), a chunk of raw
        scans in host memory at a time.  `label_map`: scannetv2-labels.combined.tsv's path, or the dict
        of scannet_raw.read_label_map.  The exported arrays stay on the host for `export`."""
        scan_names = list(scan_names)
        if not scan_names:
            raise SceneError("no scans to load from %s" % raw_dir)
        if not isinstance(label_map, dict):
            label_map = raw.read_label_map(label_map)
        records = (raw.read_raw_scan(raw_dir, s, label_map) for s in scan_names)
        exported = dict(zip(scan_names, raw.export_raw_scans(records, device, max_points, seed)))

        def read(s):
            e = exported[s]
            return scene_from_arrays(s, e["vert"], e["ins_label"], e["sem_label"], e["bbox"], use_color, use_height)

        self = cls.__new__(cls)
        self._pack(raw_dir, scan_names, read, device, use_color, use_height)
        self.raw_export = exported
        return self

    def export(self, out_dir):
        """Write `<scan>_vert.npy`, `_ins_label.npy`, `_sem_label.npy` and `_bbox.npy` of every scan of
        a from_raw store: the folder ScanNetScenes(out_dir, ...) reads."""
        if self.raw_export is None:
            raise RuntimeError("ScanNetScenes.export: only a from_raw store holds the arrays to write")
        os.makedirs(out_dir, exist_ok=True)
        for s in self.scan_names:
            raw.save_export(out_dir, s, self.raw_export[s])


# ------------------------------------------------------------------ host restatement
def host_scene(scene, idx, u=None, votes=True, boxes="raw", mean_size=None, has_height=True):
    """One scene of a batch in numpy, the reference's own arithmetic: the sample `idx`, the
    augmentation of the uniforms `u` (None: none), vote labels after it, box labels ('aug': in the
    augmented frame, 'raw': un-augmented, None: none)."""
    pc = scene["cloud"][idx].copy()
    out = {}
    tb = np.zeros((MAX_NUM_OBJ, 6))
    nb = scene["boxes"].shape[0]
    tb[:nb] = scene["boxes"][:, 0:6]
    if u is not None:
        fx, fy, angle, scale = augmentation(u)
        aug_boxes = boxes == "aug"
        if fx:
            pc[:, 0] = -1 * pc[:, 0]
            if aug_boxes:
                tb[:, 0] = -1 * tb[:, 0]
        if fy:
            pc[:, 1] = -1 * pc[:, 1]
            if aug_boxes:
                tb[:, 1] = -1 * tb[:, 1]
        rot = rotz(angle)
        pc[:, 0:3] = np.dot(pc[:, 0:3], np.transpose(rot))
        scale_ratio = np.expand_dims(np.tile(scale, 3), 0)
        pc[:, 0:3] *= scale_ratio
        if has_height:
            pc[:, -1] *= scale_ratio[0, 0]
        if aug_boxes:
            tb = rotate_aligned_boxes(tb, rot)
            tb[:, 0:3] *= scale_ratio
            tb[:, 3:6] *= scale_ratio
        out.update(flip_x_axis=fx, flip_y_axis=fy, rot_mat=rot.astype(np.float32),
                   rot_angle=np.float32(angle), scale=scale_ratio.astype(np.float32))
    else:
        out.update(flip_x_axis=0, flip_y_axis=0, rot_mat=np.identity(3, np.float32),
                   rot_angle=np.float32(0), scale=np.ones((1, 3), np.float32))
    out["point_clouds"] = pc.astype(np.float32)
    if votes:
        n = len(idx)
        inst, sem = scene["inst"][idx], scene["sem"][idx]
        point_votes = np.zeros([n, 3])
        point_votes_mask = np.zeros(n)
        for i_instance in np.unique(inst):  # scannet_ssl_dataset.py:136-147
            ind = np.where(inst == i_instance)[0]
            if sem[ind[0]] in NYU40IDS:
                x = pc[ind, :3]
                center = 0.5 * (x.min(0) + x.max(0))
                point_votes[ind, :] = center - x
                point_votes_mask[ind] = 1.0
        out["vote_label"] = np.tile(point_votes, (1, 3)).astype(np.float32)
        out["vote_label_mask"] = point_votes_mask.astype(np.int64)
    if boxes is not None:
        cls = scene["boxes"][:, 6].astype(np.int64)
        size_classes = np.zeros(MAX_NUM_OBJ, np.int64)
        size_classes[:nb] = cls
        size_residuals = np.zeros((MAX_NUM_OBJ, 3))
        size_residuals[:nb] = tb[:nb, 3:6] - mean_size[cls, :]
        mask = np.zeros(MAX_NUM_OBJ, np.float32)
        mask[:nb] = 1
        out.update(center_label=tb.astype(np.float32)[:, 0:3], size_class_label=size_classes,
                   sem_cls_label=size_classes.copy(), size_residual_label=size_residuals.astype(np.float32),
                   heading_class_label=np.zeros(MAX_NUM_OBJ, np.int64),
                   heading_residual_label=np.zeros(MAX_NUM_OBJ, np.float32), box_label_mask=mask)
    return out


# ------------------------------------------------------------------ batches
class ScanNetLoader(SceneLoader):
    """SceneLoader with the semantics of the reference's ScanNet datasets:

      pretrain_batch   ScannetDetectionDataset('train', augment=True)    (pretrain.py)
      semi_batch       ScannetSSLLabeledDataset + ScannetSSLUnlabeledDataset rows (train.py:321-325)
      eval_batch       ScannetDetectionDataset('val', augment=False)

    `config`: scannet_config(mean_size_arr=...).  Explicit draws: {'idx': (B, N) ints, 'ema_idx':
    (B, N), 'u': (B, 4) float64 uniforms}."""
    _Args, _ENTRY, _DATASET = records.SceneBatchArgs, "scene_batch_build", "scannet"
    _STORE_KEYS = ("cloud", "inst", "sem", "offset", "count", "ninst", "boxes", "nbox")
    _UNIFORMS = {"u": 4}
    _uniforms = staticmethod(uniforms)

    def _scratch(self, vote_rows):
        dev = self.scenes.device
        return {"idx": torch.empty((max(vote_rows, 1), self.num_points), dtype=torch.int32, device=dev),
                "table": torch.empty((max(vote_rows, 1), MAX_INSTANCES, 8), dtype=torch.int32, device=dev)}

    def _fill(self, a, kind, nl, given, scratch):
        if scratch["idx"].shape[0] < a.vote_rows or scratch["idx"].shape[1] != a.N:
            raise ValueError("output set's scratch is too small")
        a.idx_out, a.table = scratch["idx"].data_ptr(), scratch["table"].data_ptr()

    def _host_row(self, scene, kind, r, labeled, idx, u, boxes, draws):
        return host_scene(scene, idx, u, votes=labeled, boxes=boxes, mean_size=self.mean_size,
                          has_height=self.scenes.use_height)


def write_synthetic_scans(data_dir, names, num_points=50000, instances=40, boxes=25, seed=0):
    """Seeded ScanNet-sized stand-ins in the preprocessed layout (for tests and tools/, where no
    dataset is at hand): a room of points, `instances` instance ids with nyu40 and other semantic
    labels, `boxes` boxes."""
    g = np.random.default_rng(seed)
    other = [1, 2, 13, 40]
    for name in names:
        xyz = (g.random((num_points, 3)) * [8.0, 6.0, 3.0] - [4.0, 3.0, 0.1]).astype(np.float32)
        rgb = g.integers(0, 256, (num_points, 3)).astype(np.float32)
        inst = g.integers(0, instances, num_points).astype(np.uint32)
        labels = np.array([NYU40IDS[g.integers(0, 18)] if g.random() < 0.7 else other[g.integers(0, 4)]
                           for _ in range(instances)], np.uint32)
        box = np.zeros((boxes, 7))
        box[:, 0:3] = g.random((boxes, 3)) * [8.0, 6.0, 2.0] - [4.0, 3.0, 0.0]
        box[:, 3:6] = g.random((boxes, 3)) * 1.5 + 0.2
        box[:, 6] = NYU40IDS[g.integers(0, 18, boxes)]
        np.save(os.path.join(data_dir, name + "_vert.npy"), np.concatenate([xyz, rgb], 1))
        np.save(os.path.join(data_dir, name + "_ins_label.npy"), inst)
        np.save(os.path.join(data_dir, name + "_sem_label.npy"), labels[inst])
        np.save(os.path.join(data_dir, name + "_bbox.npy"), box)
