"""What the three batch loaders share on the host: scannet_data (ScanNet), sunrgbd_data (SUN RGB-D) and
scan_data (scans without labels).  Nothing here knows a dataset.

  draws     the counter-based hash and the point sampler in numpy (csrc/scene_common.h is the device
            form): every random quantity of a batch is a pure function of (seed, counter, row, draw)
  stores    `SceneStore`: the per-scene offset / count table, the padded box table, the upload
  loaders   `SceneLoader`: batch layout, explicit draws, the args record, the host restatement's
            skeleton; a dataset's loader overrides the few methods that are its own.  With
            `unlabeled_scans=` (a scan_data.ScanStore) the unlabeled rows of a semi batch come from
            scans without labels: the dataset's build for the leading rows, ScanLoader.semi_rows for
            the trailing ones
  launch    the ONE place that decides which stream a build's memory is recorded on
  epochs    epoch_plan, feed (builds on the train step's side stream), eval_batches

The device builders (csrc/scene_batch.hip, sunrgbd_batch.hip, scan_batch.hip) differ in their
arithmetic and stay apart; they share csrc/scene_common.h.
"""
import importlib

import numpy as np
import torch

MAX_BATCH = 64    # scenes per batch (SB_MAX_B, SUN_MAX_B, SCAN_MAX_B)
MAX_NUM_OBJ = 64  # box label rows per scene, both datasets (scannet_ssl_dataset.py:20, sunrgbd_detection_dataset.py:40)
DRAW_STUDENT, DRAW_EMA = 0, 1  # draw indices of the two point samples, the same in every header


class SceneError(ValueError):
    pass


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


def unit_uniform(keys):
    """uint32 keys -> float64 uniforms in [0, 1) (32 bits)."""
    return keys.astype(np.float64) * 2.0 ** -32


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


def explicit_indices(values, counts, num_points, key, what):
    """Explicit point indices (B, num_points) as the int32 the device reads; their bounds are checked
    here, on the host, before anything is launched."""
    v = np.asarray(values).reshape(len(counts), num_points)
    if (v < 0).any() or (v >= counts[:, None]).any():
        raise ValueError("explicit draws %r out of range of the %s point counts" % (key, what))
    return np.ascontiguousarray(v, np.int32)


def rotz(t):  # utils/pc_util.py:311-317
    c, s = np.cos(t), np.sin(t)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def _read_list(path):
    with open(path) as f:
        return [x.strip() for x in f.read().splitlines() if x.strip()]


# ------------------------------------------------------------------ the resident store
def scene_offsets(count):
    """The first row of every scene in the flat arrays (int64)."""
    return np.concatenate([[0], np.cumsum(count, dtype=np.int64)[:-1]]).astype(np.int64)


def to_device(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


class SceneStore(object):
    """Every scan of `scan_names` read once (`read(name)` -> the scene's dict with "cloud" (n, C)
    float32 and "boxes" (nb, box_cols) float64) and packed into flat device arrays with a per-scene
    offset / count table and a box table padded to MAX_NUM_OBJ rows.  `device=None` keeps the host
    copy only (the CPU path).  A dataset's store adds its own arrays to `dev`."""

    def __init__(self, data_dir, scan_names, read, device, box_cols):
        if not scan_names:
            raise SceneError("no scans to load from %s" % data_dir)
        self.scan_names = list(scan_names)
        self.scenes = [read(s) for s in self.scan_names]
        self.channels = self.scenes[0]["cloud"].shape[1]
        self.count = np.array([s["cloud"].shape[0] for s in self.scenes], np.int32)
        self.offset = scene_offsets(self.count)
        self.nbox = np.array([s["boxes"].shape[0] for s in self.scenes], np.int32)
        self.boxes = np.zeros((len(self.scenes), MAX_NUM_OBJ, box_cols))
        for i, s in enumerate(self.scenes):
            self.boxes[i, :s["boxes"].shape[0]] = s["boxes"]
        self.device = torch.device(device) if device is not None else None
        self.dev = None
        if self.device is not None:
            self.dev = {"cloud": self._flat("cloud"), "offset": self._upload(self.offset),
                        "count": self._upload(self.count), "boxes": self._upload(self.boxes),
                        "nbox": self._upload(self.nbox)}

    def _upload(self, a):
        return to_device(a, self.device)

    def _flat(self, key):
        """The scenes' per-point array `key`, one after another, on the device."""
        return self._upload(np.concatenate([s[key] for s in self.scenes]))

    def __len__(self):
        return len(self.scan_names)

    def index(self, names):
        where = {s: i for i, s in enumerate(self.scan_names)}
        return np.array([where[s] for s in names], np.int64)


# ------------------------------------------------------------------ the launch
def launch(entry, args, keep, stream, device):
    """Run the builder `entry` of the library on `stream` (None: the device's current stream) with
    the filled args record.  `keep`: the device memory the caller allocated for this call on the
    CURRENT stream and that `stream` writes or reads -- fresh outputs, scratch, uploaded draws."""
    from .. import _lib
    current = torch.cuda.current_stream(device)
    if stream is None:
        stream = current
    if keep and stream != current:
        stream.wait_stream(current)  # the blocks just allocated may have been freed by queued work
    _lib.run(entry, args, device, stream=stream.cuda_stream)
    for t in keep:  # not handed to another allocation before `stream` is done with them
        t.record_stream(stream)


# ------------------------------------------------------------------ host restatement: stacking rows
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
def _sizes(labeled_ids, unlabeled_ids):
    return np.size(labeled_ids), 0 if unlabeled_ids is None else np.size(unlabeled_ids)


class SceneLoader(object):
    """Batches of `num_points` points per scene from the store `scenes`:

      pretrain_batch   the detection dataset, 'train', augment=True
      semi_batch       labeled rows, then unlabeled rows (student and teacher sample of each)
      eval_batch       the detection dataset, 'val', augment=False

    `labeled` / `unlabeled`: the scan names of each list (default: every scan of the store); ids
    passed to the builders index these lists and are what scan_idx reports.  `config.mean_size_arr`
    gives the size residuals, in float64 as the reference.  Device draws are keyed by (seed, counter,
    batch row, draw index); `draws=` replaces them with explicit ones.

    A dataset's loader sets `_Args` (its args record, a class of records.py), `_ENTRY` (the library's
    builder), `_STORE_KEYS` (the store's device arrays, named as the record's fields), `_UNIFORMS`
    (explicit per-row uniforms: key -> how many; draw `key` goes to the field `key_in`) and
    `_uniforms` (seed, counter, row -> the row's augmentation uniforms), and overrides `_host_row`
    and, where it has something to add, `_scratch`, `_given`, `_fill`, `_extra_host_draws` and
    `_teacher_colour`.

    `unlabeled_scans`: a scan_data.ScanStore of the loader's `_DATASET` on the scenes' device.  The
    unlabeled list is then that store -- scans WITHOUT label files -- and `unlabeled_ids` index it: a
    semi batch is the dataset's own build of the labeled rows into the leading rows of the batch's
    tensors and ScanLoader.semi_rows into the trailing ones, on one stream.  For scans stored as
    float32 files the batch is bit-equal to the one this loader gives with the same scans in its
    labeled store.  Such a batch has no labels for its unlabeled rows (unlabeled_labels=True raises)
    and needs a labeled row in front."""
    _UNIFORMS = {}
    _DATASET = None

    def __init__(self, scenes, config, num_points, seed=0, labeled=None, unlabeled=None, unlabeled_scans=None):
        self.scenes, self.config, self.num_points, self.seed = scenes, config, int(num_points), int(seed)
        self.mean_size = np.asarray(getattr(config, "mean_size_arr_f64", config.mean_size_arr), np.float64)
        self.labeled = scenes.index(labeled) if labeled is not None else np.arange(len(scenes))
        self.unlabeled_scans = self._scan_rows = None
        if unlabeled_scans is not None:
            if unlabeled is not None:
                raise ValueError("unlabeled_scans is the unlabeled list: give it or `unlabeled`, not both")
            self._adopt(unlabeled_scans)
            self.unlabeled = np.arange(len(unlabeled_scans))
        else:
            self.unlabeled = scenes.index(unlabeled) if unlabeled is not None else np.arange(len(scenes))
        self._mean_dev = None
        if scenes.device is not None:
            self._mean_dev = to_device(self.mean_size, scenes.device)

    def _adopt(self, store):
        scan_data = importlib.import_module(__package__ + ".scan_data")  # (it imports this module)
        if store.dataset != self._DATASET:
            raise ValueError("unlabeled_scans holds %r scans, this is a %r loader" % (store.dataset, self._DATASET))
        if store.device != self.scenes.device:
            raise ValueError("unlabeled_scans is on %s, the labeled scenes are on %s"
                             % (store.device, self.scenes.device))
        if self.scenes.use_color and store.columns != 6:
            raise ValueError("the labeled scenes use colour, unlabeled_scans holds 3-column clouds (xyz only)")
        self.unlabeled_scans = store
        self._scan_rows = scan_data.ScanLoader(store, self.num_points, use_color=self.scenes.use_color,
                                               use_height=self.scenes.use_height, seed=self.seed)

    def _mixed(self, kind, nl, nu, unlabeled_labels):
        """Does a batch take its unlabeled rows from `unlabeled_scans`?  Refuses what such a batch
        cannot be."""
        if kind != "semi" or self.unlabeled_scans is None:
            return False
        if unlabeled_labels:
            raise ValueError("unlabeled_labels=True: the scans of unlabeled_scans have no labels to give")
        if nl == 0:
            raise ValueError("a semi batch over unlabeled_scans needs at least one labeled row")
        if nl + nu > MAX_BATCH:
            raise ValueError("a batch holds 1..%d scenes, got %d" % (MAX_BATCH, nl + nu))
        return nu > 0

    @staticmethod
    def _split_draws(draws, nl):
        """Explicit draws of a mixed batch -> (the labeled rows', the unlabeled rows')."""
        if draws is None:
            return None, None
        lab = {k: np.asarray(v)[:nl] for k, v in draws.items()}
        return lab, {k: np.asarray(draws[k])[nl:] for k in ("idx", "ema_idx", "u") if k in draws}

    # ---------------------------------------------------------------- layouts
    def _layout(self, kind, nl, nu=0, unlabeled_labels=False):
        self._mixed(kind, nl, nu, unlabeled_labels)
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
        """One output set (batch tensors, the builder's scratch) on the store's device."""
        shapes, vote_rows, _ = self._layout(kind, nl, nu, unlabeled_labels)
        dev = self.scenes.device
        return {k: torch.empty(s, dtype=d, device=dev) for k, (s, d) in shapes.items()}, self._scratch(vote_rows)

    def _scratch(self, vote_rows):
        return {}

    # ---------------------------------------------------------------- device builds
    def _rows(self, kind, labeled_ids, unlabeled_ids):
        lab = np.asarray(labeled_ids, np.int64).reshape(-1)
        unl = np.asarray(unlabeled_ids if unlabeled_ids is not None else [], np.int64).reshape(-1)
        if kind == "semi":
            scene = np.concatenate([self.labeled[lab], self.unlabeled[unl]])
        else:
            scene = self.labeled[lab]
        scan_idx = np.concatenate([lab, unl])
        if not 1 <= len(scene) <= MAX_BATCH:
            raise ValueError("a batch holds 1..%d scenes, got %d" % (MAX_BATCH, len(scene)))
        return scene, scan_idx, len(lab), len(unl)

    def _given(self, draws, counts):
        """The explicit draws of a build as the contiguous arrays the device reads."""
        given = {}
        for key in ("idx", "ema_idx"):
            if key in draws:
                given[key] = explicit_indices(draws[key], counts, self.num_points, key, "scenes'")
        for key, k in self._UNIFORMS.items():
            if key in draws:
                given[key] = np.ascontiguousarray(np.asarray(draws[key], np.float64).reshape(len(counts), k))
        return given

    def _fill(self, a, kind, nl, given, scratch):
        """The record's fields that only this dataset has."""

    def build(self, kind, labeled_ids, unlabeled_ids=None, counter=0, unlabeled_labels=False,
              out=None, draws=None, stream=None):
        """One batch of `kind` ('pretrain' | 'semi' | 'eval') on the device, into the output set `out`
        (None: freshly allocated) on `stream` (None: the current stream)."""
        if self._mixed(kind, *_sizes(labeled_ids, unlabeled_ids), unlabeled_labels):
            return self._build_mixed(labeled_ids, unlabeled_ids, counter, out, draws, stream)
        scene, scan_idx, nl, nu = self._rows(kind, labeled_ids, unlabeled_ids)
        B, N = len(scene), self.num_points
        given = self._given(draws, self.scenes.count[scene]) if draws is not None else {}
        if self.scenes.dev is None:
            raise RuntimeError("%s: the store has no device copy (device=None); use host_batch"
                               % type(self).__name__)
        shapes, vote_rows, box_rows = self._layout(kind, nl, nu, unlabeled_labels)
        fresh = out is None
        if fresh:
            out = self.allocate(kind, nl, nu, unlabeled_labels)
        batch, scratch = out
        for k, (s, d) in shapes.items():
            if k not in batch or tuple(batch[k].shape) != s or batch[k].dtype != d:
                raise ValueError("output set does not match the batch layout at %r" % k)
        a = self._Args()
        a.B, a.N, a.C = B, N, self.scenes.channels
        a.has_height = int(self.scenes.use_height)
        a.augment = int(kind != "eval")
        a.ema = int(kind == "semi")
        a.vote_rows, a.box_rows = vote_rows, box_rows
        a.box_aug_rows = vote_rows if kind != "eval" else 0
        a.NS = self.mean_size.shape[0]
        a.seed, a.counter = self.seed & 0xFFFFFFFF, int(counter) & 0xFFFFFFFF
        for r in range(B):
            a.scene[r], a.scan_idx[r], a.supervised[r] = int(scene[r]), int(scan_idx[r]), int(r < nl)
        self._fill(a, kind, nl, given, scratch)
        for k in self._STORE_KEYS:
            setattr(a, k, self.scenes.dev[k].data_ptr())
        a.mean_size = self._mean_dev.data_ptr()
        keep = []
        for key, v in given.items():
            t = to_device(v, self.scenes.device)
            keep.append(t)
            setattr(a, key + "_in", t.data_ptr())
        if fresh:
            keep += list(batch.values()) + list(scratch.values())
        for k in shapes:
            setattr(a, "scan_idx_out" if k == "scan_idx" else k, batch[k].data_ptr())
        launch(self._ENTRY, a, keep, stream, self.scenes.device)
        result = dict(batch)
        result["supervised_mask_host"] = tuple([1] * nl + [0] * nu)
        return result

    _build = build  # the loaders' GPU tests call the builder by this name

    def _build_mixed(self, labeled_ids, unlabeled_ids, counter, out, draws, stream):
        """A semi batch whose unlabeled rows come from `unlabeled_scans`: ScanLoader's launch into the
        trailing rows, then this dataset's own launches for the leading ones, on the same stream."""
        lab = np.asarray(labeled_ids, np.int64).reshape(-1)
        unl = np.asarray(unlabeled_ids, np.int64).reshape(-1)
        nl, nu = len(lab), len(unl)
        if self.scenes.dev is None:
            raise RuntimeError("%s: the store has no device copy (device=None); use host_batch"
                               % type(self).__name__)
        shapes, _, _ = self._layout("semi", nl, nu)
        fresh = out is None
        if fresh:
            out = self.allocate("semi", nl, nu)
        batch, scratch = out
        for k, (s, d) in shapes.items():
            if k not in batch or tuple(batch[k].shape) != s or batch[k].dtype != d:
                raise ValueError("output set does not match the batch layout at %r" % k)
        lab_draws, unl_draws = self._split_draws(draws, nl)
        tail = {k: batch[k][nl:] for k in self._scan_rows._SEMI_KEYS}
        keep = list(batch.values()) + list(scratch.values()) if fresh else []
        self._scan_rows._semi_launch(unl, counter, nl, tail, unl_draws, stream, keep)
        # the leading rows of every tensor: the labeled build sees a batch of nl rows, keyed by row
        self.build("semi", lab, None, counter, out=({k: batch[k][:nl] for k in shapes}, scratch),
                   draws=lab_draws, stream=stream)
        result = dict(batch)
        result["supervised_mask_host"] = tuple([1] * nl + [0] * nu)
        return result

    def pretrain_batch(self, ids, counter=0, out=None, draws=None, stream=None):
        return self.build("pretrain", ids, None, counter, out=out, draws=draws, stream=stream)

    def semi_batch(self, labeled_ids, unlabeled_ids, counter=0, unlabeled_labels=False, out=None,
                   draws=None, stream=None):
        return self.build("semi", labeled_ids, unlabeled_ids, counter, unlabeled_labels, out=out,
                          draws=draws, stream=stream)

    def eval_batch(self, ids, counter=0, out=None, draws=None, stream=None):
        return self.build("eval", ids, None, counter, out=out, draws=draws, stream=stream)

    # ---------------------------------------------------------------- the host restatement
    def _extra_host_draws(self, draws, kind, counter, n):
        """The dataset's draws beyond idx / ema_idx / u, added to `draws` (n: the rows' point counts)."""

    def host_draws(self, kind, labeled_ids, unlabeled_ids=None, counter=0):
        """The device's own draws of a batch, on the host (exact)."""
        if self._mixed(kind, *_sizes(labeled_ids, unlabeled_ids), False):
            draws = self.host_draws(kind, labeled_ids, None, counter)
            tail = self._scan_rows.host_semi_draws(unlabeled_ids, counter, np.size(labeled_ids))
            return {k: np.concatenate([draws[k], tail[k]]) for k in ("idx", "ema_idx", "u")}
        scene, _, nl, nu = self._rows(kind, labeled_ids, unlabeled_ids)
        B, N = len(scene), self.num_points
        n = self.scenes.count[scene]
        draws = {"idx": np.stack([sample_indices(self.seed, counter, r, DRAW_STUDENT, n[r], N) for r in range(B)])}
        if kind == "semi":
            draws["ema_idx"] = np.stack([sample_indices(self.seed, counter, r, DRAW_EMA, n[r], N)
                                         for r in range(B)])
        if kind != "eval":
            draws["u"] = np.stack([self._uniforms(self.seed, counter, r) for r in range(B)])
        self._extra_host_draws(draws, kind, counter, n)
        return draws

    def _host_row(self, scene, kind, r, labeled, idx, u, boxes, draws):
        """The dataset's host_scene for batch row r of `kind`."""
        raise NotImplementedError

    def _teacher_colour(self, ema, labeled):
        """The teacher's sample of a semi row, after the colour normalisation of its dataset."""
        return ema

    def host_batch(self, kind, labeled_ids, unlabeled_ids=None, counter=0, unlabeled_labels=False,
                   draws=None):
        """numpy restatement of pretrain_batch / semi_batch / eval_batch (kind = 'pretrain' | 'semi' |
        'eval'): the same outputs for the same draws (default: the device's, host_draws)."""
        if self._mixed(kind, *_sizes(labeled_ids, unlabeled_ids), unlabeled_labels):
            lab_draws, unl_draws = self._split_draws(draws, np.size(labeled_ids))
            out = self.host_batch(kind, labeled_ids, None, counter, draws=lab_draws)
            tail = self._scan_rows.host_semi_rows(unlabeled_ids, counter, np.size(labeled_ids), unl_draws)
            for k, v in tail.items():
                out[k] = np.concatenate([out[k], v])
            return out
        scene, scan_idx, nl, nu = self._rows(kind, labeled_ids, unlabeled_ids)
        if draws is None:
            draws = self.host_draws(kind, labeled_ids, unlabeled_ids, counter)
        rows = []
        for r, s in enumerate(scene):
            sc = self.scenes.scenes[s]
            u = np.asarray(draws["u"])[r] if kind != "eval" else None
            lab = r < nl
            box = ("aug" if kind != "eval" else "raw") if lab else ("raw" if unlabeled_labels else None)
            row = self._host_row(sc, kind, r, lab, np.asarray(draws["idx"][r]), u, box, draws)
            if kind == "semi":
                ema = sc["cloud"][np.asarray(draws["ema_idx"][r])].astype(np.float32)
                row["ema_point_clouds"] = self._teacher_colour(ema, lab)
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
        b = loader.build(kind, lab, unl, counter, unlabeled_labels, out=sets[s], stream=side)
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
