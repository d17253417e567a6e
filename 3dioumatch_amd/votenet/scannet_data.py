"""ScanNet train / eval batches built on the GPU from a resident scene store.

The reference's loaders (scannet/scannet_ssl_dataset.py:47-184, :224-320 and
scannet/scannet_detection_dataset.py:85-223) redo per-scene numpy work in every __getitem__: two
random subsets, flip / rotate / scale, a Python loop over the instances for the vote labels.
Here the preprocessed scans (`<scan>_vert.npy`, `_ins_label.npy`, `_sem_label.npy`, `_bbox.npy`,
as batch_load_scannet_data.py writes them) are read ONCE into flat device arrays
(`ScanNetScenes`), and a batch is three kernel launches (csrc/scene_batch.hip, include/scene_hip.h)
on the train step's side stream (`feed`), so no step waits on the host.

Every random draw is a counter-based hash of (seed, batch counter, batch row, draw index); a batch
is a pure function of its arguments.  `host_*` below restate the whole construction in numpy --
the same hash, the same bijection, the reference's own float64 / float32 arithmetic -- which is the
CPU path and the yardstick of the device path.

Keys, dtypes and shapes are those of data.make_batch (pretrain, eval) and data.make_semi_batch
(semi-supervised); semi batches also carry `supervised_mask_host`.
"""
import ctypes
import importlib
import os

import numpy as np
import torch

MAX_NUM_OBJ = 64      # scannet_ssl_dataset.py:20
MAX_INSTANCES = 1024  # dense instance ids per scene (SB_MAX_INST)
MAX_BATCH = 64        # scenes per batch (SB_MAX_B)
MEAN_COLOR_RGB = np.array([109.8, 97.2, 83.8])  # scannet_ssl_dataset.py:21
NYU40IDS = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39])  # model_util_scannet.py:30
DRAW_STUDENT, DRAW_EMA, DRAW_UNIFORM = 0, 1, 2  # draw indices of the hash (scene_hip.h)

_c_int, _c_uint, _vp = ctypes.c_int, ctypes.c_uint, ctypes.c_void_p


# ------------------------------------------------------------------ counter-based draws (host form)
def _u32(x):
    return np.atleast_1d(np.asarray(x, dtype=np.uint64) & 0xFFFFFFFF).astype(np.uint32)


def mix32(h):
    """murmur3's finaliser on uint32 arrays (wrapping arithmetic, as on the device)."""
    h = _u32(h)
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x85EBCA6B)
    h = h ^ (h >> np.uint32(13))
    h = h * np.uint32(0xC2B2AE35)
    return h ^ (h >> np.uint32(16))


def draw_key(seed, counter, row, draw):
    h = mix32(_u32(seed) * np.uint32(0x9E3779B9) + np.uint32(0x85EBCA6B))
    h = mix32(h ^ (_u32(counter) * np.uint32(0xC2B2AE35) + np.uint32(0x27D4EB2F)))
    h = mix32(h ^ (_u32(row) * np.uint32(0x165667B1) + np.uint32(0xD3A2646C)))
    return mix32(h ^ (_u32(draw) * np.uint32(0xFD7046C5) + np.uint32(0xB55A4F09)))


def _element(key, j):
    return mix32(_u32(key) ^ (_u32(j) * np.uint32(0x9E3779B9) + np.uint32(0x7F4A7C15)))


def _feistel(x, h, key):
    mask = np.uint32((1 << h) - 1)
    l, r = x >> np.uint32(h), x & mask
    for rnd in range(4):
        f = mix32(r ^ _element(key, rnd)) & mask
        l, r = r, l ^ f
    return (l << np.uint32(h)) | r


def _half_bits(n):
    h = 1
    while h < 15 and (1 << (2 * h)) < n:
        h += 1
    return h


def sample_indices(seed, counter, row, draw, n, num_points):
    """The device's point sample of one (row, draw): `num_points` DISTINCT indices of [0, n) when
    n >= num_points (a keyed 4-round Feistel bijection of [0, 4^h) restricted to [0, n) by cycle
    walking, slots 0..num_points-1), i.i.d. with replacement otherwise (pc_util.random_sampling:
    replace = n < N)."""
    key = draw_key(seed, counter, row, draw)
    j = np.arange(num_points, dtype=np.uint32)
    if n < num_points:
        return ((_element(key, j).astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)
    h = _half_bits(n)
    x = _feistel(j, h, key)
    walk = x >= n
    while walk.any():
        x[walk] = _feistel(x[walk], h, key)
        walk = x >= n
    return x.astype(np.int64)


def uniforms(seed, counter, row):
    """The four uniforms in [0, 1) of a row: flip x, flip y, angle, scale (float64, 32 bits)."""
    keys = draw_key(seed, counter, row, DRAW_UNIFORM + np.arange(4))
    return keys.astype(np.float64) * 2.0 ** -32


def augmentation(u):
    """uniforms -> (flip_x, flip_y, angle, scale) with the reference's formulas
    (scannet_ssl_dataset.py:102-124)."""
    return (int(u[0] > 0.5), int(u[1] > 0.5), (u[2] * np.pi / 18) - np.pi / 36, u[3] * 0.3 + 0.85)


def rotz(t):  # utils/pc_util.py:311-317
    c, s = np.cos(t), np.sin(t)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


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
class SceneError(ValueError):
    pass


def read_scene(data_dir, name, use_color=False, use_height=True):
    """One preprocessed scan -> the per-scene state the batches are built from, computed once:
    cloud (n, C) float32 = xyz, [(rgb - MEAN_COLOR_RGB) / 256], [z - floor]; the floor height
    (np.percentile(z, 0.99) of the raw cloud, as every __getitem__ of the reference recomputes it);
    dense instance ids; semantic ids; the box table (nb, 7) float64 = centre, size, class index."""
    paths = {k: os.path.join(data_dir, name + "_%s.npy" % k) for k in ("vert", "ins_label", "sem_label", "bbox")}
    for k, p in paths.items():
        if not os.path.exists(p):
            raise SceneError("scan %s: missing %s" % (name, p))
    vert = np.load(paths["vert"])
    ins = np.load(paths["ins_label"]).reshape(-1)
    sem = np.load(paths["sem_label"]).reshape(-1)
    bbox = np.load(paths["bbox"])
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


def _read_list(path):
    with open(path) as f:
        return [x.strip() for x in f.read().splitlines() if x.strip()]


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
class ScanNetScenes(object):
    """Every scan of `scan_names` read once and packed into flat device arrays with a per-scene
    offset / count table (the whole ScanNet train split is ~1.5 GB at <= 50k points per scan).
    `device=None` keeps the host copy only (the CPU path)."""

    def __init__(self, data_dir, scan_names, device, use_color=False, use_height=True):
        if not scan_names:
            raise SceneError("no scans to load from %s" % data_dir)
        self.scan_names = list(scan_names)
        self.use_color, self.use_height = use_color, use_height
        self.scenes = [read_scene(data_dir, s, use_color, use_height) for s in self.scan_names]
        self.channels = self.scenes[0]["cloud"].shape[1]
        self.count = np.array([s["cloud"].shape[0] for s in self.scenes], np.int32)
        self.offset = np.concatenate([[0], np.cumsum(self.count, dtype=np.int64)[:-1]]).astype(np.int64)
        self.ninst = np.array([s["ninst"] for s in self.scenes], np.int32)
        self.nbox = np.array([s["boxes"].shape[0] for s in self.scenes], np.int32)
        self.floor = np.array([s["floor"] for s in self.scenes], np.float32)
        self.boxes = np.zeros((len(self.scenes), MAX_NUM_OBJ, 7))
        for i, s in enumerate(self.scenes):
            self.boxes[i, :s["boxes"].shape[0]] = s["boxes"]
        self.device = torch.device(device) if device is not None else None
        self.dev = None
        if self.device is not None:
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)  # noqa: E731
            self.dev = {
                "cloud": t(np.concatenate([s["cloud"] for s in self.scenes])),
                "inst": t(np.concatenate([s["inst"] for s in self.scenes])),
                "sem": t(np.concatenate([s["sem"] for s in self.scenes])),
                "offset": t(self.offset), "count": t(self.count), "ninst": t(self.ninst),
                "boxes": t(self.boxes), "nbox": t(self.nbox),
            }

    def __len__(self):
        return len(self.scan_names)

    def index(self, names):
        where = {s: i for i, s in enumerate(self.scan_names)}
        return np.array([where[s] for s in names], np.int64)


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


_BOX_KEYS = ("center_label", "heading_class_label", "heading_residual_label", "size_class_label",
             "size_residual_label", "sem_cls_label", "box_label_mask")
_DRAW_KEYS = ("flip_x_axis", "flip_y_axis", "rot_mat", "rot_angle", "scale")


_EMPTY = {"vote_label": ((9,), np.float32), "vote_label_mask": ((), np.int64),
          "center_label": ((MAX_NUM_OBJ, 3), np.float32), "heading_class_label": ((MAX_NUM_OBJ,), np.int64),
          "heading_residual_label": ((MAX_NUM_OBJ,), np.float32), "size_class_label": ((MAX_NUM_OBJ,), np.int64),
          "size_residual_label": ((MAX_NUM_OBJ, 3), np.float32), "sem_cls_label": ((MAX_NUM_OBJ,), np.int64),
          "box_label_mask": ((MAX_NUM_OBJ,), np.float32)}


def _stack(rows, keys, num_points=0):
    out = {}
    for k in keys:
        if not rows:  # no labeled row: (0, ...) tensors, as the device batch has
            shape, dtype = _EMPTY[k]
            lead = (0, num_points) if k.startswith("vote") else (0,)
            out[k] = np.zeros(lead + shape, dtype)
            continue
        v = np.stack([np.asarray(r[k]) for r in rows])
        out[k] = v.astype(np.int64) if k in ("flip_x_axis", "flip_y_axis") else v
    return out


# ------------------------------------------------------------------ batches
class _Args(ctypes.Structure):  # field order == include/scene_hip.h SceneBatchArgs
    _fields_ = ([(n, _c_int) for n in ("B", "N", "C", "has_height", "augment", "ema", "vote_rows",
                                       "box_rows", "box_aug_rows", "NS")] +
                [("seed", _c_uint), ("counter", _c_uint)] +
                [(n, _c_int * MAX_BATCH) for n in ("scene", "scan_idx", "supervised")] +
                [(n, _vp) for n in ("cloud", "inst", "sem", "offset", "count", "ninst", "boxes", "nbox",
                                    "mean_size", "idx_in", "ema_idx_in", "u_in", "idx_out", "table",
                                    "point_clouds", "ema_point_clouds", "vote_label", "vote_label_mask",
                                    "center_label", "heading_class_label", "heading_residual_label",
                                    "size_class_label", "size_residual_label", "sem_cls_label",
                                    "box_label_mask", "supervised_mask", "scan_idx_out", "flip_x_axis",
                                    "flip_y_axis", "rot_angle", "rot_mat", "scale")])


class ScanNetLoader(object):
    """Batches of `num_points` points per scene from `scenes`, with the semantics of the reference's
    datasets:

      pretrain_batch   ScannetDetectionDataset('train', augment=True)    (pretrain.py)
      semi_batch       ScannetSSLLabeledDataset + ScannetSSLUnlabeledDataset rows (train.py:321-325)
      eval_batch       ScannetDetectionDataset('val', augment=False)

    `labeled` / `unlabeled`: the scan names of each list (default: every scan of the store); ids
    passed to the builders index these lists and are what scan_idx reports.  `config.mean_size_arr`
    (scannet_config(mean_size_arr=...)) gives the size residuals, in float64 as the reference.
    Device draws are keyed by (seed, counter, batch row, draw index); `draws=` replaces them with
    explicit ones: {'idx': (B, N) ints, 'ema_idx': (B, N), 'u': (B, 4) float64 uniforms}."""

    def __init__(self, scenes, config, num_points, seed=0, labeled=None, unlabeled=None):
        self.scenes, self.config, self.num_points, self.seed = scenes, config, int(num_points), int(seed)
        self.mean_size = np.asarray(getattr(config, "mean_size_arr_f64", config.mean_size_arr), np.float64)
        self.labeled = scenes.index(labeled) if labeled is not None else np.arange(len(scenes))
        self.unlabeled = scenes.index(unlabeled) if unlabeled is not None else np.arange(len(scenes))
        self._mean_dev = None
        if scenes.device is not None:
            self._mean_dev = torch.from_numpy(np.ascontiguousarray(self.mean_size)).to(scenes.device)

    # ---------------------------------------------------------------- layouts
    def _layout(self, kind, nl, nu=0, unlabeled_labels=False):
        N, C = self.num_points, self.scenes.channels
        B = nl + nu
        f, i64 = torch.float32, torch.int64
        shapes = {"point_clouds": ((B, N, C), f), "supervised_mask": ((B,), i64), "scan_idx": ((B,), i64)}
        vote_rows = nl
        box_rows = B if (kind == "semi" and unlabeled_labels) else nl
        shapes.update({"vote_label": ((vote_rows, N, 9), f), "vote_label_mask": ((vote_rows, N), i64),
                       "center_label": ((box_rows, MAX_NUM_OBJ, 3), f),
                       "heading_class_label": ((box_rows, MAX_NUM_OBJ), i64),
                       "heading_residual_label": ((box_rows, MAX_NUM_OBJ), f),
                       "size_class_label": ((box_rows, MAX_NUM_OBJ), i64),
                       "size_residual_label": ((box_rows, MAX_NUM_OBJ, 3), f),
                       "sem_cls_label": ((box_rows, MAX_NUM_OBJ), i64),
                       "box_label_mask": ((box_rows, MAX_NUM_OBJ), f)})
        if kind == "semi":
            shapes.update({"ema_point_clouds": ((B, N, C), f), "flip_x_axis": ((B,), i64),
                           "flip_y_axis": ((B,), i64), "rot_angle": ((B,), f), "rot_mat": ((B, 3, 3), f),
                           "scale": ((B, 1, 3), f)})
        return shapes, vote_rows, box_rows

    def allocate(self, kind, nl, nu=0, unlabeled_labels=False):
        """One output set (batch tensors + the builder's scratch) on the store's device."""
        shapes, vote_rows, _ = self._layout(kind, nl, nu, unlabeled_labels)
        dev = self.scenes.device
        batch = {k: torch.empty(s, dtype=d, device=dev) for k, (s, d) in shapes.items()}
        scratch = {"idx": torch.empty((max(vote_rows, 1), self.num_points), dtype=torch.int32, device=dev),
                   "table": torch.empty((max(vote_rows, 1), MAX_INSTANCES, 8), dtype=torch.int32, device=dev)}
        return batch, scratch

    # ---------------------------------------------------------------- device builds
    def _rows(self, kind, labeled_ids, unlabeled_ids):
        lab = np.asarray(labeled_ids, np.int64).reshape(-1)
        unl = np.asarray(unlabeled_ids if unlabeled_ids is not None else [], np.int64).reshape(-1)
        lst_l = self.labeled
        if kind == "semi":
            scene = np.concatenate([lst_l[lab], self.unlabeled[unl]])
        else:
            scene = lst_l[lab]
        scan_idx = np.concatenate([lab, unl])
        if not 1 <= len(scene) <= MAX_BATCH:
            raise ValueError("a batch holds 1..%d scenes, got %d" % (MAX_BATCH, len(scene)))
        return scene, scan_idx, len(lab), len(unl)

    def _build(self, kind, labeled_ids, unlabeled_ids=None, counter=0, unlabeled_labels=False,
               out=None, draws=None, stream=None):
        scene, scan_idx, nl, nu = self._rows(kind, labeled_ids, unlabeled_ids)
        B, N, C = len(scene), self.num_points, self.scenes.channels
        given = {}
        if draws is not None:  # bounds: checked on the host before anything is launched
            counts = self.scenes.count[scene]
            for key in ("idx", "ema_idx"):
                if key in draws:
                    v = np.asarray(draws[key]).reshape(B, N)
                    if (v < 0).any() or (v >= counts[:, None]).any():
                        raise ValueError("explicit draws %r out of range of the scenes' point counts" % key)
                    given[key] = np.ascontiguousarray(v, np.int32)
            if "u" in draws:
                given["u"] = np.ascontiguousarray(np.asarray(draws["u"], np.float64).reshape(B, 4))
        if self.scenes.dev is None:
            raise RuntimeError("ScanNetLoader: the store has no device copy (device=None); use host_batch")
        _L = importlib.import_module("3dioumatch_amd._lib")
        shapes, vote_rows, box_rows = self._layout(kind, nl, nu, unlabeled_labels)
        current = torch.cuda.current_stream(self.scenes.device)
        if stream is None:
            stream = current
        fresh = out is None
        if fresh:
            out = self.allocate(kind, nl, nu, unlabeled_labels)
        batch, scratch = out
        for k, (s, d) in shapes.items():
            if k not in batch or tuple(batch[k].shape) != s or batch[k].dtype != d:
                raise ValueError("output set does not match the batch layout at %r" % k)
        if scratch["idx"].shape[0] < vote_rows or scratch["idx"].shape[1] != N:
            raise ValueError("output set's scratch is too small")
        a = _Args()
        a.B, a.N, a.C = B, N, C
        a.has_height = int(self.scenes.use_height)
        a.augment = int(kind != "eval")
        a.ema = int(kind == "semi")
        a.vote_rows, a.box_rows = vote_rows, box_rows
        a.box_aug_rows = vote_rows if kind != "eval" else 0
        a.NS = self.mean_size.shape[0]
        a.seed, a.counter = self.seed & 0xFFFFFFFF, int(counter) & 0xFFFFFFFF
        for r in range(B):
            a.scene[r], a.scan_idx[r], a.supervised[r] = int(scene[r]), int(scan_idx[r]), int(r < nl)
        d = self.scenes.dev
        for k in ("cloud", "inst", "sem", "offset", "count", "ninst", "boxes", "nbox"):
            setattr(a, k, d[k].data_ptr())
        a.mean_size = self._mean_dev.data_ptr()
        keep = []  # device memory this call allocates on the current stream and `stream` writes or reads
        for key, field in (("idx", "idx_in"), ("ema_idx", "ema_idx_in"), ("u", "u_in")):
            if key in given:
                t = torch.from_numpy(given[key]).to(self.scenes.device)
                keep.append(t)
                setattr(a, field, t.data_ptr())
        if fresh:
            keep += list(batch.values()) + list(scratch.values())
        a.idx_out, a.table = scratch["idx"].data_ptr(), scratch["table"].data_ptr()
        for k in ("point_clouds", "ema_point_clouds", "vote_label", "vote_label_mask", "center_label",
                  "heading_class_label", "heading_residual_label", "size_class_label",
                  "size_residual_label", "sem_cls_label", "box_label_mask", "supervised_mask",
                  "flip_x_axis", "flip_y_axis", "rot_angle", "rot_mat", "scale"):
            if k in batch:
                setattr(a, k, batch[k].data_ptr())
        a.scan_idx_out = batch["scan_idx"].data_ptr()
        if keep and stream != current:
            stream.wait_stream(current)  # the blocks just allocated may have been freed by queued work
        with torch.cuda.device(self.scenes.device):
            _L.check(_L.lib.scene_batch_build(ctypes.byref(a), stream.cuda_stream), "scene_batch_build")
        for t in keep:  # not handed to another allocation before `stream` is done with them
            t.record_stream(stream)
        result = dict(batch)
        result["supervised_mask_host"] = tuple([1] * nl + [0] * nu)
        return result

    def pretrain_batch(self, ids, counter=0, out=None, draws=None, stream=None):
        return self._build("pretrain", ids, None, counter, out=out, draws=draws, stream=stream)

    def semi_batch(self, labeled_ids, unlabeled_ids, counter=0, unlabeled_labels=False, out=None,
                   draws=None, stream=None):
        return self._build("semi", labeled_ids, unlabeled_ids, counter, unlabeled_labels, out=out,
                           draws=draws, stream=stream)

    def eval_batch(self, ids, counter=0, out=None, draws=None, stream=None):
        return self._build("eval", ids, None, counter, out=out, draws=draws, stream=stream)

    # ---------------------------------------------------------------- the host restatement
    def host_draws(self, kind, labeled_ids, unlabeled_ids=None, counter=0):
        """The device's own draws of a batch, on the host (exact)."""
        scene, _, nl, nu = self._rows(kind, labeled_ids, unlabeled_ids)
        B, N = len(scene), self.num_points
        n = self.scenes.count[scene]
        draws = {"idx": np.stack([sample_indices(self.seed, counter, r, DRAW_STUDENT, n[r], N) for r in range(B)])}
        if kind == "semi":
            draws["ema_idx"] = np.stack([sample_indices(self.seed, counter, r, DRAW_EMA, n[r], N)
                                         for r in range(B)])
        if kind != "eval":
            draws["u"] = np.stack([uniforms(self.seed, counter, r) for r in range(B)])
        return draws

    def host_batch(self, kind, labeled_ids, unlabeled_ids=None, counter=0, unlabeled_labels=False,
                   draws=None):
        """numpy restatement of pretrain_batch / semi_batch / eval_batch (kind = 'pretrain' | 'semi' |
        'eval'): the same outputs for the same draws (default: the device's, host_draws)."""
        scene, scan_idx, nl, nu = self._rows(kind, labeled_ids, unlabeled_ids)
        if draws is None:
            draws = self.host_draws(kind, labeled_ids, unlabeled_ids, counter)
        hh = self.scenes.use_height
        rows = []
        for r, s in enumerate(scene):
            sc = self.scenes.scenes[s]
            u = draws["u"][r] if kind != "eval" else None
            lab = r < nl
            box = ("aug" if kind != "eval" else "raw") if lab else ("raw" if unlabeled_labels else None)
            row = host_scene(sc, np.asarray(draws["idx"][r]), u, votes=lab, boxes=box,
                             mean_size=self.mean_size, has_height=hh)
            if kind == "semi":
                row["ema_point_clouds"] = sc["cloud"][np.asarray(draws["ema_idx"][r])].astype(np.float32)
            rows.append(row)
        out = _stack(rows, ["point_clouds"])
        out.update(_stack(rows[:nl], ("vote_label", "vote_label_mask"), self.num_points))
        box_rows = nl + nu if (kind == "semi" and unlabeled_labels) else nl
        out.update(_stack(rows[:box_rows], _BOX_KEYS))
        if kind == "semi":
            out.update(_stack(rows, ("ema_point_clouds",) + _DRAW_KEYS))
            out["rot_angle"] = out["rot_angle"].astype(np.float32)
        out["supervised_mask"] = np.array([1] * nl + [0] * nu, np.int64)
        out["scan_idx"] = scan_idx.astype(np.int64)
        return out


# ------------------------------------------------------------------ epochs and feeding
def epoch_plan(num_labeled, batch_size, epoch, seed=0, num_unlabeled=0, unlabeled_batch_size=0,
               rank=0, world=1):
    """The batches of one epoch as (counter, labeled_ids, unlabeled_ids) (unlabeled_ids None without
    an unlabeled list).  A seeded shuffle per epoch, the same on every rank, rank r taking r::world of
    it (DistributedSampler); the labeled list drives the epoch and the unlabeled order restarts, with
    a fresh shuffle, when it runs out (train.py:312-319).

    Deviation from the reference: a trailing partial batch is DROPPED -- a new batch size would
    re-capture the step's graphs -- and every rank gets the same number of batches."""
    def order(n, stream, round_):
        perm = np.random.default_rng([seed, epoch, stream, round_]).permutation(n)
        return perm[rank::world][: n // world]

    lab = order(num_labeled, 0, 0)
    steps = len(lab) // batch_size
    unl, unl_round, pos = None, 0, 0
    if num_unlabeled:
        if num_unlabeled // world < unlabeled_batch_size:
            raise ValueError("fewer unlabeled scenes per rank than one unlabeled batch")
        unl = order(num_unlabeled, 1, 0)
    for i in range(steps):
        u_ids = None
        if unl is not None:
            if pos + unlabeled_batch_size > len(unl):
                unl_round += 1
                unl, pos = order(num_unlabeled, 1, unl_round), 0
            u_ids = unl[pos:pos + unlabeled_batch_size]
            pos += unlabeled_batch_size
        counter = (epoch * steps + i) * world + rank
        yield counter, lab[i * batch_size:(i + 1) * batch_size], u_ids


def feed(runner, loader, plan, kind="semi", unlabeled_labels=False):
    """Yield the batches of `plan` (epoch_plan: every batch of one layout) built on the device and
    ready for `runner`: batch i+1 is built on runner.side_stream() into one of three output sets,
    its index chain is prefetched (runner.prefetch_geometry), then batch i is yielded.  The caller
    runs the step on the yielded batch before asking for the next one.

    Stream discipline: the three sets are allocated up front, on the main stream, and the side
    stream then waits for everything main has queued -- so no set can be a block that a step still
    in flight on main has freed.  A set is rebuilt only after an event recorded on main behind the
    step that consumed it.  When the generator ends or is closed early, main waits for the side
    stream, so the sets go back to the allocator only behind every build and prefetch that used
    them."""
    if kind not in ("pretrain", "semi"):
        raise ValueError("feed builds training batches; eval batches come from eval_batches")
    device = loader.scenes.device
    side = runner.side_stream()
    main = torch.cuda.current_stream(device)
    it = iter(plan)
    try:
        first = next(it)
    except StopIteration:
        return
    nl, nu = len(first[1]), 0 if first[2] is None else len(first[2])
    sets = [loader.allocate(kind, nl, nu, unlabeled_labels) for _ in range(3)]
    built, consumed = [torch.cuda.Event() for _ in range(3)], [None] * 3
    side.wait_stream(main)  # the sets' blocks, the store's upload, whatever else main has queued

    def build(i, item):
        counter, lab, unl = item
        s = i % 3
        if consumed[s] is not None:
            side.wait_event(consumed[s])
        b = loader._build(kind, lab, unl, counter, unlabeled_labels, out=sets[s], stream=side)
        built[s].record(side)
        return b

    try:
        nxt = build(0, first)
        runner.prefetch_geometry(nxt)
        i = 0
        while nxt is not None:
            cur = nxt
            try:
                nxt = build(i + 1, next(it))
                runner.prefetch_geometry(nxt)
            except StopIteration:
                nxt = None
            main.wait_event(built[i % 3])
            yield cur
            ev = torch.cuda.Event()
            ev.record(main)
            consumed[i % 3] = ev
            i += 1
    finally:
        main.wait_stream(side)


def eval_batches(loader, batch_size, counter=0):
    """Every scene of the loader's labeled list in order, batch_size at a time (the last batch may
    be smaller), freshly allocated on the current stream (inference.evaluate keeps the list)."""
    n = len(loader.labeled)
    for i, start in enumerate(range(0, n, batch_size)):
        yield loader.eval_batch(np.arange(start, min(n, start + batch_size)), counter + i)


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
