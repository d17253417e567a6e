"""Scans WITHOUT labels: a resident store of raw clouds and the eval batches built from it on the GPU.

Both labeled stores (scannet_data.ScanNetScenes, sunrgbd_data.SunRgbdScenes) refuse a scan without
its label files.  `ScanStore` takes bare (n, 3) xyz or (n, 6) xyz + rgb clouds -- arrays, `.npy`
files, `.npz` files with a `pc` member (the SUN RGB-D `_pc.npz` layout), `.ply` meshes' vertices or
`.mat` depth clouds (the raw SUN RGB-D `depth/` layout) -- keeps the RAW float32
rows in one flat device array with an offset / count table, and does in ONE launch at construction
(scene_scan_prepare, include/scan_hip.h) everything that needs a pass over the points: the floor
height np.percentile(z, 0.99) of every scan and its count of non-finite values.  The constructor reads
that small table once -- the only host read of the store's life -- and raises for a NaN or Inf.

`ScanLoader.batch` is one launch (scene_scan_batch_build): the eval sampling of the labeled loaders
(the same counter-based draw, so the same rows for the same (seed, counter, ids)), the dataset's
colour normalisation rounded once from double as read_scene does, and height = z - floor in float32.
`host_floor` and `ScanLoader.host_batch` restate both in numpy: the CPU path and the yardstick.
The draw, the bounds check of explicit indices and the launch with its stream discipline are
scene_loader's, the same functions the labeled loaders use.

`ScanLoader.semi_rows` is one launch too (scene_scan_semi_build): the UNLABELED rows of a
semi-supervised batch -- the student's sample through the dataset's flip / rotation / scale in the
labeled kernels' arithmetic, the teacher's sample, the row header -- keyed by the rows' place behind
the batch's labeled rows (`row0`), so that scene_loader.SceneLoader(unlabeled_scans=store) can put them
behind its own labeled rows; `host_semi_rows` is the numpy restatement.

One difference from the SUN RGB-D reader: float64 input is cast to float32 on the host BEFORE the
floor and the colour normalisation, where sunrgbd_data.read_scene works in the file's dtype and
rounds afterwards.  For float32 files (and every ScanNet `_vert.npy`, which the ScanNet reader casts
first too) the batches are bit-equal to the labeled loaders' eval batches.

Zero sign: -0.0 and +0.0 compare equal in numpy's partition, so where the selected order statistic is
a zero its sign is unspecified; floors are compared with ==, everything else bit for bit.
"""
import os

import numpy as np
import torch

from .. import records
from .scannet_raw import read_ply_vertices
from .sunrgbd_raw import read_mat_points
from .scene_loader import (DRAW_EMA, DRAW_STUDENT, MAX_BATCH, SceneError, draw_key, epoch_plan,  # noqa: F401
                           eval_batches, explicit_indices, feed, launch, rotz, sample_indices, scene_offsets,
                           to_device, unit_uniform)

DATASETS = ("scannet", "sunrgbd")
MEAN_COLOR_RGB = {"scannet": np.array([109.8, 97.2, 83.8]),  # scannet_detection_dataset.py:24
                  "sunrgbd": np.array([0.5, 0.5, 0.5])}      # sunrgbd_detection_dataset.py:41


def host_floor(z):
    """np.percentile(z.astype(float32), 0.99) restated: the two order statistics of numpy's linear
    method and its float32 interpolation (numpy.lib._function_base_impl._quantile / _lerp), every
    operation rounded to float32.  Bit-equal to np.percentile apart from the sign of a zero."""
    z = np.asarray(z, np.float32).reshape(-1)
    n = z.shape[0]
    if n == 0:
        raise ValueError("host_floor: an empty cloud")
    f = np.float32
    q = f(0.99) / f(100)
    v = f(q * f(n - 1))
    lo = min(int(np.floor(v)), n - 1)
    hi = min(lo + 1, n - 1)
    g = f(v - f(lo))
    part = np.partition(z, sorted({lo, hi}))
    a, b = part[lo], part[hi]
    d = f(b - a)
    if g >= f(0.5):
        return f(b - f(d * f(f(1) - g)))
    return f(a + f(d * g))


DRAW_UNIFORM = 2  # draw index of the first augmentation uniform of a row (scene_hip.h, sunrgbd_hip.h)
UNIFORMS = {"scannet": 4,   # flip x, flip y, angle, scale
            "sunrgbd": 3}   # flip, angle, scale


def augmentation(dataset, u):
    """A row's uniforms -> (flip_x, flip_y, angle, scale) with the formulas of the dataset's unlabeled
    loader (scannet_ssl_dataset.py:258-280: +-5 degrees; sunrgbd_ssl_dataset.py:259-281: no y flip,
    +-30 degrees)."""
    if dataset == "scannet":
        return int(u[0] > 0.5), int(u[1] > 0.5), (u[2] * np.pi / 18) - np.pi / 36, u[3] * 0.3 + 0.85
    return int(u[0] > 0.5), 0, (u[1] * np.pi / 3) - np.pi / 6, u[2] * 0.3 + 0.85


def _load_cloud(path):
    name = os.path.basename(path)
    for suffix in ("_vert.npy", "_pc.npz", ".npy", ".npz", ".ply", ".mat"):
        if name.endswith(suffix):
            name = name[:-len(suffix)]
            break
    if not os.path.exists(path):
        raise SceneError("scan %s: missing %s" % (name, path))
    if path.endswith(".npz"):
        with np.load(path) as f:
            if "pc" not in f.files:
                raise SceneError("scan %s: %s has no 'pc'" % (name, path))
            return name, f["pc"]
    if path.endswith(".npy"):
        return name, np.load(path)
    if path.endswith(".ply"):  # xyz or xyz rgb as the file has them: aligning a mesh is the caller's job
        return name, read_ply_vertices(path)
    if path.endswith(".mat"):  # a SUN RGB-D depth cloud: the variable `instance`, xyz or xyz rgb
        return name, read_mat_points(path, columns=(3, 6))
    raise SceneError("scan %s: %s is neither .npy, .npz, .ply nor .mat" % (name, path))


def scan_prepare_gpu(cloud, offset, count):
    """(floor (S,) f32, nonfinite (S,) i32) of the scans of a flat (P, C) device cloud: one launch."""
    from .. import _lib
    S = count.shape[0]
    floor = torch.empty(S, dtype=torch.float32, device=cloud.device)
    nonfinite = torch.empty(S, dtype=torch.int32, device=cloud.device)
    a = records.ScanPrepareArgs()
    a.S, a.C = S, cloud.shape[1]
    a.cloud, a.offset, a.count = cloud.data_ptr(), offset.data_ptr(), count.data_ptr()
    a.floor, a.nonfinite = floor.data_ptr(), nonfinite.data_ptr()
    _lib.run("scene_scan_prepare", a, cloud.device)
    return floor, nonfinite


class ScanStore(object):
    """`clouds`: a list of (n_i, 3) or (n_i, 6) arrays (xyz, optionally rgb), 1 <= n_i < 2^30, all of
    one width; float64 is cast to float32 here (see the module docstring).  The raw rows live in one
    flat device array; `device=None` keeps the host copy only (the CPU path: floors by host_floor).
    Malformed input raises SceneError naming the scan."""

    def __init__(self, clouds, device, dataset="scannet", names=None):
        if dataset not in DATASETS:
            raise ValueError("dataset must be one of %s, got %r" % (DATASETS, dataset))
        clouds = list(clouds)
        if not clouds:
            raise SceneError("no scans to load")
        self.names = list(names) if names is not None else ["scan%04d" % i for i in range(len(clouds))]
        if len(self.names) != len(clouds) or len(set(self.names)) != len(clouds):
            raise ValueError("names: one distinct name per cloud")
        self.dataset = dataset
        rows = []
        for name, c in zip(self.names, clouds):
            c = np.asarray(c)
            if c.ndim != 2:
                raise SceneError("scan %s: the cloud has shape %s, expected (n, 3) or (n, 6)" % (name, c.shape))
            if c.shape[1] not in (3, 6):
                raise SceneError("scan %s: %d columns, expected 3 (xyz) or 6 (xyz rgb)" % (name, c.shape[1]))
            if c.shape[0] == 0 or c.shape[0] >= 1 << 30:
                raise SceneError("scan %s: %d points" % (name, c.shape[0]))
            if c.dtype.kind not in "fiu":
                raise SceneError("scan %s: dtype %s is not numeric" % (name, c.dtype))
            rows.append(np.ascontiguousarray(c, np.float32))
        self.columns = rows[0].shape[1]
        for name, c in zip(self.names, rows):
            if c.shape[1] != self.columns:
                raise SceneError("scan %s: %d columns, but scan %s has %d (one width per store)"
                                 % (name, c.shape[1], self.names[0], self.columns))
        self.clouds = rows
        self.count = np.array([c.shape[0] for c in rows], np.int32)
        self.offset = scene_offsets(self.count)
        self.device = torch.device(device) if device is not None else None
        self.dev = None
        if self.device is None:
            nonfinite = np.array([int((~np.isfinite(c)).sum()) for c in rows], np.int64)
            self._refuse(nonfinite)
            self.floor = np.array([host_floor(c[:, 2]) for c in rows], np.float32)
            return
        self.dev = {"cloud": to_device(np.concatenate(rows), self.device),
                    "offset": to_device(self.offset, self.device), "count": to_device(self.count, self.device)}
        floor, nonfinite = scan_prepare_gpu(self.dev["cloud"], self.dev["offset"], self.dev["count"])
        self.dev["floor"] = floor
        table = torch.stack([floor.double(), nonfinite.double()]).cpu().numpy()  # the one host read
        self._refuse(table[1].astype(np.int64))
        self.floor = table[0].astype(np.float32)

    def _refuse(self, nonfinite):
        bad = ["%s (%d)" % (self.names[i], nonfinite[i]) for i in np.nonzero(nonfinite)[0]]
        if bad:
            raise SceneError("scans with NaN or Inf coordinates or colours (count): " + ", ".join(bad))

    @classmethod
    def from_files(cls, paths, device, dataset="scannet", names=None):
        """`.npy` files, `.npz` files with a `pc` member, `.ply` files (the vertices' x y z, with red
        green blue when the file has them, through scannet_raw.read_ply_vertices; the coordinates are
        used as they are) and `.mat` files (SUN RGB-D depth clouds: the variable `instance`, through
        sunrgbd_raw.read_mat_points); the default names are the file names without `_vert.npy` /
        `_pc.npz` / the extension."""
        loaded = [_load_cloud(p) for p in paths]
        if names is None:
            names = [n for n, _ in loaded]
        return cls([c for _, c in loaded], device, dataset, names)

    def __len__(self):
        return len(self.names)


class ScanLoader(object):
    """Batches of `num_points` points per scan: {'point_clouds': (B, N, 3 + C) f32, 'scan_idx': (B,)
    i64}, the rows ScannetDetectionDataset / SunrgbdDetectionDataset('val', augment=False) give for a
    scan (scannet_detection_dataset.py:85-223, sunrgbd_detection_dataset.py:119-246) without their
    labels.  The sample of row r is the draw (seed, counter, r, DRAW_STUDENT) of the labeled
    loaders; `draws={'idx': (B, N) ints}` replaces it.  With use_color=False a 6-column store
    serves xyz only."""

    def __init__(self, store, num_points, use_color=False, use_height=True, seed=0):
        if use_color and store.columns != 6:
            raise ValueError("ScanLoader: use_color needs a store of 6-column clouds (xyz rgb)")
        self.store, self.num_points, self.seed = store, int(num_points), int(seed)
        if self.num_points < 1:
            raise ValueError("ScanLoader: num_points >= 1")
        self.use_color, self.use_height = bool(use_color), bool(use_height)
        self.channels = 3 + 3 * self.use_color + self.use_height

    def __len__(self):
        return len(self.store)

    def _ids(self, ids):
        ids = np.asarray(ids, np.int64).reshape(-1)
        if not 1 <= len(ids) <= MAX_BATCH:
            raise ValueError("a batch holds 1..%d scans, got %d" % (MAX_BATCH, len(ids)))
        if (ids < 0).any() or (ids >= len(self.store)).any():
            raise ValueError("scan ids out of range of the store's %d scans" % len(self.store))
        return ids

    def _given(self, ids, draws):
        return explicit_indices(draws["idx"], self.store.count[ids], self.num_points, "idx", "scans'")

    def allocate(self, B):
        dev = self.store.device
        return {"point_clouds": torch.empty((B, self.num_points, self.channels), dtype=torch.float32, device=dev),
                "scan_idx": torch.empty((B,), dtype=torch.int64, device=dev)}

    def batch(self, ids, counter=0, out=None, draws=None, stream=None):
        ids = self._ids(ids)
        B, N = len(ids), self.num_points
        given = self._given(ids, draws) if draws is not None and "idx" in draws else None
        st = self.store
        if st.dev is None:
            raise RuntimeError("ScanLoader: the store has no device copy (device=None); use host_batch")
        fresh = out is None
        if fresh:
            out = self.allocate(B)
        pc, si = out["point_clouds"], out["scan_idx"]
        if tuple(pc.shape) != (B, N, self.channels) or pc.dtype != torch.float32 or not pc.is_contiguous() or \
                tuple(si.shape) != (B,) or si.dtype != torch.int64 or pc.device != st.device:
            raise ValueError("output set does not match the batch layout")
        a = records.ScanBatchArgs()
        a.B, a.N, a.C = B, N, st.columns
        a.use_color, a.use_height = int(self.use_color), int(self.use_height)
        a.dataset = DATASETS.index(st.dataset)
        a.seed, a.counter = self.seed & 0xFFFFFFFF, int(counter) & 0xFFFFFFFF
        for r in range(B):
            a.scene[r], a.scan_idx[r] = int(ids[r]), int(ids[r])
        for k in ("cloud", "offset", "count", "floor"):
            setattr(a, k, st.dev[k].data_ptr())
        keep = [pc, si] if fresh else []
        if given is not None:
            keep.append(to_device(given, st.device))
            a.idx_in = keep[-1].data_ptr()
        a.point_clouds, a.scan_idx_out = pc.data_ptr(), si.data_ptr()
        launch("scene_scan_batch_build", a, keep, stream, st.device)
        return {"point_clouds": pc, "scan_idx": si}

    def batches(self, batch_size, counter=0):
        """Every scan of the store in order, batch_size at a time (the last batch may be smaller),
        batch i with counter + i."""
        n = len(self.store)
        for i, start in enumerate(range(0, n, batch_size)):
            yield self.batch(np.arange(start, min(n, start + batch_size)), counter + i)

    # ---------------------------------------------------------------- the host restatement
    def host_draws(self, ids, counter=0):
        ids = self._ids(ids)
        n = self.store.count[ids]
        return {"idx": np.stack([sample_indices(self.seed, counter, r, DRAW_STUDENT, n[r], self.num_points)
                                 for r in range(len(ids))])}

    def host_batch(self, ids, counter=0, draws=None):
        """numpy restatement of batch(): the same outputs for the same draws (default: the device's)."""
        ids = self._ids(ids)
        idx = self._given(ids, draws) if draws is not None and "idx" in draws else self.host_draws(ids, counter)["idx"]
        rows = [self._host_rows(s, idx[r]) for r, s in enumerate(ids)]
        return {"point_clouds": np.stack(rows), "scan_idx": ids.astype(np.int64)}

    def _host_rows(self, s, idx):
        """The points `idx` of scan s as eval rows: xyz, [normalised rgb], [z - floor]."""
        st = self.store
        raw = st.clouds[s][idx]
        cols = [raw[:, 0:3]]
        if self.use_color:
            rgb = raw[:, 3:6] - MEAN_COLOR_RGB[st.dataset]  # float32 - float64: double
            if st.dataset == "scannet":
                rgb = rgb / 256.0
            cols.append(rgb.astype(np.float32))
        if self.use_height:
            cols.append((raw[:, 2] - np.float32(st.floor[s]))[:, None])
        return np.concatenate(cols, 1).astype(np.float32)

    # ---------------------------------------------------------------- unlabeled rows of a semi batch
    _SEMI_KEYS = ("point_clouds", "ema_point_clouds", "flip_x_axis", "flip_y_axis", "rot_angle", "rot_mat",
                  "scale", "supervised_mask", "scan_idx")

    def _semi_layout(self, B):
        N, C = self.num_points, self.channels
        f, i64 = torch.float32, torch.int64
        return {"point_clouds": ((B, N, C), f), "ema_point_clouds": ((B, N, C), f), "flip_x_axis": ((B,), i64),
                "flip_y_axis": ((B,), i64), "rot_angle": ((B,), f), "rot_mat": ((B, 3, 3), f),
                "scale": ((B, 1, 3), f), "supervised_mask": ((B,), i64), "scan_idx": ((B,), i64)}

    def allocate_semi(self, B):
        dev = self.store.device
        return {k: torch.empty(s, dtype=d, device=dev) for k, (s, d) in self._semi_layout(B).items()}

    def _row0(self, row0, B):
        row0 = int(row0)
        if row0 < 0 or row0 + B > MAX_BATCH:
            raise ValueError("row0 = %d: %d rows behind it pass the batch limit of %d" % (row0, B, MAX_BATCH))
        return row0

    def _given_semi(self, ids, draws):
        """The explicit draws of semi_rows as the contiguous arrays the device reads."""
        given = {}
        for key in ("idx", "ema_idx"):
            if key in draws:
                given[key] = explicit_indices(draws[key], self.store.count[ids], self.num_points, key, "scans'")
        if "u" in draws:
            given["u"] = np.ascontiguousarray(
                np.asarray(draws["u"], np.float64).reshape(len(ids), UNIFORMS[self.store.dataset]))
        return given

    def semi_rows(self, ids, counter=0, row0=0, out=None, draws=None, stream=None):
        """The UNLABELED rows of a semi-supervised batch for the scans `ids`, one launch
        (scene_scan_semi_build): {'point_clouds' (the student's sample, augmented), 'ema_point_clouds'
        (the teacher's, not augmented), 'flip_x_axis', 'flip_y_axis', 'rot_angle', 'rot_mat', 'scale',
        'supervised_mask' (zeros), 'scan_idx'}, the rows the labeled loaders' semi_batch gives behind
        its `row0` labeled rows: the draws of row r are keyed by batch row row0 + r.  `out`: a dict of
        these tensors with len(ids) rows (trailing-row views of a batch's tensors will do).  Explicit
        draws: 'idx', 'ema_idx' (B, N) and 'u' (B, 4) for ScanNet, (B, 3) for SUN RGB-D."""
        return self._semi_launch(ids, counter, row0, out, draws, stream, [])

    def _semi_launch(self, ids, counter, row0, out, draws, stream, keep):
        """semi_rows; `keep`: more memory of the caller's that scene_loader.launch is to treat as
        allocated for this call (the rest of a freshly allocated mixed batch)."""
        ids = self._ids(ids)
        B, N = len(ids), self.num_points
        row0 = self._row0(row0, B)
        given = self._given_semi(ids, draws) if draws is not None else {}
        st = self.store
        if st.dev is None:
            raise RuntimeError("ScanLoader: the store has no device copy (device=None); use host_semi_rows")
        keep = list(keep)
        if out is None:
            out = self.allocate_semi(B)
            keep += list(out.values())
        for k, (s, d) in self._semi_layout(B).items():
            if k not in out or tuple(out[k].shape) != s or out[k].dtype != d or not out[k].is_contiguous() or \
                    out[k].device != st.device:
                raise ValueError("output set does not match the rows' layout at %r" % k)
        a = records.ScanSemiArgs()
        a.B, a.N, a.C, a.row0 = B, N, st.columns, row0
        a.use_color, a.use_height = int(self.use_color), int(self.use_height)
        a.dataset = DATASETS.index(st.dataset)
        a.seed, a.counter = self.seed & 0xFFFFFFFF, int(counter) & 0xFFFFFFFF
        for r in range(B):
            a.scene[r], a.scan_idx[r] = int(ids[r]), int(ids[r])
        for k in ("cloud", "offset", "count", "floor"):
            setattr(a, k, st.dev[k].data_ptr())
        for key, v in given.items():
            keep.append(to_device(v, st.device))
            setattr(a, key + "_in", keep[-1].data_ptr())
        for k in self._SEMI_KEYS:
            setattr(a, "scan_idx_out" if k == "scan_idx" else k, out[k].data_ptr())
        launch("scene_scan_semi_build", a, keep, stream, st.device)
        return {k: out[k] for k in self._SEMI_KEYS}

    def host_semi_draws(self, ids, counter=0, row0=0):
        """The device's own draws of semi_rows, on the host (exact)."""
        ids = self._ids(ids)
        row0 = self._row0(row0, len(ids))
        n, N = self.store.count[ids], self.num_points
        rows = range(len(ids))
        return {"idx": np.stack([sample_indices(self.seed, counter, row0 + r, DRAW_STUDENT, n[r], N) for r in rows]),
                "ema_idx": np.stack([sample_indices(self.seed, counter, row0 + r, DRAW_EMA, n[r], N) for r in rows]),
                "u": np.stack([unit_uniform(draw_key(self.seed, counter, row0 + r, DRAW_UNIFORM +
                                                     np.arange(UNIFORMS[self.store.dataset]))) for r in rows])}

    def host_semi_rows(self, ids, counter=0, row0=0, draws=None):
        """numpy restatement of semi_rows(), in the arithmetic of the reference's unlabeled datasets
        (scannet_ssl_dataset.py:224-320, sunrgbd_ssl_dataset.py:221-312; a float32 cloud, float64
        rotation matrix and scale): the same outputs for the same draws (default, and for every key
        `draws` leaves out: the device's)."""
        ids = self._ids(ids)
        d = self.host_semi_draws(ids, counter, row0)
        if draws is not None:
            d.update(self._given_semi(ids, draws))
        sun_colour = self.store.dataset == "sunrgbd" and self.use_color
        out = {k: [] for k in self._SEMI_KEYS[:7]}
        for r, s in enumerate(ids):
            pc, ema = self._host_rows(s, d["idx"][r]), self._host_rows(s, d["ema_idx"][r])
            if sun_colour:  # the unlabeled dataset's second division (sunrgbd_ssl_dataset.py:240)
                pc[:, 3:6] = pc[:, 3:6] / 256.0
                ema[:, 3:6] = ema[:, 3:6] / 256.0
            fx, fy, angle, scale = augmentation(self.store.dataset, d["u"][r])
            if fx:
                pc[:, 0] = -1 * pc[:, 0]
            if fy:
                pc[:, 1] = -1 * pc[:, 1]
            rot = rotz(angle)
            pc[:, 0:3] = np.dot(pc[:, 0:3], np.transpose(rot))
            scale_ratio = np.expand_dims(np.tile(scale, 3), 0)
            pc[:, 0:3] *= scale_ratio
            if self.use_height:
                pc[:, -1] *= scale_ratio[0, 0]
            for k, v in (("point_clouds", pc), ("ema_point_clouds", ema), ("flip_x_axis", fx), ("flip_y_axis", fy),
                         ("rot_angle", np.float32(angle)), ("rot_mat", rot.astype(np.float32)),
                         ("scale", scale_ratio.astype(np.float32))):
                out[k].append(v)
        out = {k: np.stack(v) for k, v in out.items()}
        for k in ("flip_x_axis", "flip_y_axis"):
            out[k] = out[k].astype(np.int64)
        out["rot_angle"] = out["rot_angle"].astype(np.float32)
        out["supervised_mask"] = np.zeros(len(ids), np.int64)
        out["scan_idx"] = ids.astype(np.int64)
        return out


def synthetic_clouds(count, num_points, seed=0, dataset="scannet", color=True):
    """Seeded room-sized stand-in clouds (for tools/ and tests, where no data is at hand)."""
    g = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        xyz = g.random((num_points, 3)) * [8.0, 6.0, 3.0] - [4.0, 3.0, 0.1]
        if not color:
            out.append(xyz.astype(np.float32))
            continue
        rgb = g.integers(0, 256, (num_points, 3)).astype(np.float64) if dataset == "scannet" else g.random((num_points, 3))
        out.append(np.concatenate([xyz, rgb], 1).astype(np.float32))
    return out
