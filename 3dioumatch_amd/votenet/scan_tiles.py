"""Scans larger than a room: a resident store of overlapping room-sized crops, cut on the device.

    big = ScanStore.from_files(paths, "cuda:0")              # floors of a building, registered scans
    tiles = TileStore.from_store(big, tile=(8.0, 8.0), overlap=1.0)
    found = detect_tiled(engine, tiles, config_dict)          # votenet/detect.py: one set of boxes per scan

The network sees coordinates only as differences and as z - floor, so a room-sized window of a big scan
is a legitimate input in the scan's own frame.  `TileStore` is a `ScanStore` whose scans are the windows
(`ScanLoader` and `detect` take it unchanged) and which remembers each window's parent, window and core.

The grid (`tile_grid`, float64 on the host, a few numbers per scan).  Per scan and per axis, with
L = max - min and t the tile size: one window where L <= t, else n = ceil((L - overlap) / (t - overlap))
windows with starts min + i (L - t) / (n - 1): spread evenly, the last one ending at max, the
effective overlap never below the nominal one.  Window i is [start_i, start_i + t), rounded once to
float32, the first lower bound -inf and the last upper bound +inf.  The CORE of window i -- the part of
the axis whose detections the window owns -- is [cut_(i-1), cut_i) with cut_i = (start_i + start_(i+1) +
t) / 2, the middle of the overlap of windows i and i + 1, rounded once to float32; the outermost cuts
are -inf and +inf.  So the cores partition the axis, a window contains its core, and every cut lies
overlap / 2 inside both windows it separates.  A tile is a pair (iy, ix), row-major; its window and
core are the products over the two axes.  z is not tiled.

Construction on the device (include/scan_tile_hip.h): scene_scan_bounds (two launches), the host reads
the (S, 4) bounds and makes the grid; scene_scan_tile_count, the host reads the (tiles, segments) counts
-- the second and last read -- drops the tiles below `min_points` and forms every output row from
them; scene_scan_tile_gather writes the crops (a stable compaction: the parent's rows in the parent's
order, all columns bit for bit); scene_scan_prepare gives every crop its own floor.  `host_tiles` is
the numpy restatement -- store.clouds[s][mask] with the mask written as the four compares -- and the
path of a `device=None` parent.

Dropped tiles keep their cores: a detection whose centre falls into the core of a tile that was not
built (fewer than min_points points there) is owned by no tile.
"""
import numpy as np
import torch

from .. import records
from .scan_data import ScanStore, host_floor, scan_prepare_gpu
from .scene_loader import scene_offsets, to_device

SEGMENT = 65536   # SCAN_TILE_SEGMENT
BLOCK = 1024      # SCAN_TILE_BLOCK
MAX_TILES = 4096  # SCAN_TILE_MAX

# ---------------------------------------------------------------------------------- the grid
def _tile_sizes(tile):
    t = np.asarray(tile, np.float64).reshape(-1)
    if t.shape[0] == 1:
        t = np.repeat(t, 2)
    if t.shape[0] != 2 or not np.isfinite(t).all() or (t <= 0).any():
        raise ValueError("tile: one or two sizes in metres, each > 0, got %r" % (tile,))
    return float(t[0]), float(t[1])


def _check_overlap(tx, ty, overlap):
    overlap = float(overlap)
    if not 0 <= overlap <= min(tx, ty) / 2:
        raise ValueError("overlap = %r: 0 <= overlap <= min(tile) / 2 = %r" % (overlap, min(tx, ty) / 2))
    return overlap


def axis_windows(lo, hi, t, overlap):
    """One axis of one scan: (wlo, whi, clo, chi), float32 arrays of n windows [wlo, whi) and their
    cores [clo, chi) for the extent [lo, hi], tile size t and nominal overlap (module docstring)."""
    lo, hi, t, overlap = float(lo), float(hi), float(t), float(overlap)
    inf = np.float32(np.inf)
    L = hi - lo
    if not L > t:  # (an empty or one-point extent too)
        one = np.array([inf], np.float32)
        return -one, one, -one, one
    n = int(np.ceil((L - overlap) / (t - overlap)))
    start = lo + np.arange(n, dtype=np.float64) * ((L - t) / (n - 1))
    wlo, whi = start.astype(np.float32), (start + t).astype(np.float32)
    cut = ((start[:-1] + start[1:] + t) / 2).astype(np.float32)
    wlo[0], whi[-1] = -inf, inf
    return wlo, whi, np.concatenate([[-inf], cut]).astype(np.float32), np.concatenate([cut, [inf]]).astype(np.float32)


def tile_grid(bounds, tile, overlap, names=None):
    """The tiles of S scans from their `bounds` (S, 4) = xmin, xmax, ymin, ymax: a dict of
        parent (T,) i32, iy, ix (T,) i32, window (T, 4) f32 = wlo_x, whi_x, wlo_y, whi_y,
        core (T, 4) f32 = clo_x, chi_x, clo_y, chi_y, first, tiles (S,) i32, shape (S, 2) = ny, nx,
    the tiles of a scan one after another, row-major in (iy, ix).  `names` name the scans in errors."""
    tx, ty = _tile_sizes(tile)
    overlap = _check_overlap(tx, ty, overlap)
    bounds = np.asarray(bounds, np.float32).reshape(-1, 4)
    parent, iy, ix, window, core, shape = [], [], [], [], [], []
    for s, b in enumerate(bounds.astype(np.float64)):
        xw = axis_windows(b[0], b[1], tx, overlap)
        yw = axis_windows(b[2], b[3], ty, overlap)
        nx, ny = len(xw[0]), len(yw[0])
        if nx * ny > MAX_TILES:
            raise ValueError("scan %s: %d x %d tiles of %g m x %g m, at most %d per scan"
                             % (names[s] if names is not None else s, ny, nx, tx, ty, MAX_TILES))
        jy, jx = np.divmod(np.arange(ny * nx), nx)
        parent.append(np.full(ny * nx, s, np.int32))
        iy.append(jy.astype(np.int32))
        ix.append(jx.astype(np.int32))
        window.append(np.stack([xw[0][jx], xw[1][jx], yw[0][jy], yw[1][jy]], 1))
        core.append(np.stack([xw[2][jx], xw[3][jx], yw[2][jy], yw[3][jy]], 1))
        shape.append((ny, nx))
    tiles = np.array([len(p) for p in parent], np.int32)
    return {"parent": np.concatenate(parent), "iy": np.concatenate(iy), "ix": np.concatenate(ix),
            "window": np.concatenate(window).astype(np.float32), "core": np.concatenate(core).astype(np.float32),
            "first": scene_offsets(tiles).astype(np.int32), "tiles": tiles, "shape": np.array(shape, np.int32)}


def in_box(xy, box):
    """The four compares: lo_x <= x < hi_x and lo_y <= y < hi_y in float32; box = lo_x, hi_x, lo_y, hi_y."""
    xy = np.asarray(xy, np.float32)
    b = np.asarray(box, np.float32)
    x, y = xy[..., 0], xy[..., 1]
    return (b[0] <= x) & (x < b[1]) & (b[2] <= y) & (y < b[3])


def host_bounds(clouds):
    """(S, 4) float32 xmin, xmax, ymin, ymax: scene_scan_bounds restated."""
    return np.array([[c[:, 0].min(), c[:, 0].max(), c[:, 1].min(), c[:, 1].max()] for c in clouds], np.float32)


def select_tiles(grid, counts, min_points):
    """The tiles that are built, as indices into the grid: those with at least max(min_points, 1) rows;
    a scan all of whose tiles fall short keeps the one with the most rows (the first of them)."""
    counts = np.asarray(counts, np.int64)
    keep = counts >= max(int(min_points), 1)
    for s in range(len(grid["tiles"])):
        a, b = int(grid["first"][s]), int(grid["first"][s] + grid["tiles"][s])
        if not keep[a:b].any():
            keep[a + int(np.argmax(counts[a:b]))] = True
    return np.nonzero(keep)[0]


def host_tiles(clouds, grid, min_points=1):
    """numpy restatement of the construction: (built, crops) -- the grid's tiles that are built and
    for each the parent's rows inside its window, clouds[parent][mask], in the parent's order."""
    masks = [in_box(clouds[p], w) for p, w in zip(grid["parent"], grid["window"])]
    built = select_tiles(grid, [m.sum() for m in masks], min_points)
    return built, [clouds[grid["parent"][t]][masks[t]] for t in built]


# ---------------------------------------------------------------------------------- the launches
def _segments(count):
    return max(1, -(-int(np.max(count)) // SEGMENT))


def scan_bounds_gpu(cloud, offset, count, max_segments):
    """(S, 4) float32 xmin, xmax, ymin, ymax of the scans of a flat (P, C) device cloud: two launches."""
    from .. import _lib
    S = count.shape[0]
    partial = torch.empty((S, max_segments, 4), dtype=torch.float32, device=cloud.device)
    bounds = torch.empty((S, 4), dtype=torch.float32, device=cloud.device)
    a = records.ScanBoundsArgs()
    a.S, a.C, a.max_segments = S, cloud.shape[1], max_segments
    a.cloud, a.offset, a.count = cloud.data_ptr(), offset.data_ptr(), count.data_ptr()
    a.partial, a.bounds = partial.data_ptr(), bounds.data_ptr()
    _lib.run("scene_scan_bounds", a, cloud.device)
    return bounds


def tile_count_gpu(cloud, offset, count, parent, window, max_segments):
    """(T, max_segments) int32: per tile and segment of its parent the rows inside the window."""
    from .. import _lib
    T = parent.shape[0]
    counts = torch.empty((T, max_segments), dtype=torch.int32, device=cloud.device)
    a = records.ScanTileCountArgs()
    a.T, a.C, a.max_segments = T, cloud.shape[1], max_segments
    a.cloud, a.offset, a.count = cloud.data_ptr(), offset.data_ptr(), count.data_ptr()
    a.parent, a.window, a.counts = parent.data_ptr(), window.data_ptr(), counts.data_ptr()
    _lib.run("scene_scan_tile_count", a, cloud.device)
    return counts


def tile_gather_gpu(cloud, offset, count, parent, window, base, rows, max_segments):
    """(rows, C) float32: the crops, segment g of tile t written from row base[t, g] on."""
    from .. import _lib
    crops = torch.empty((rows, cloud.shape[1]), dtype=torch.float32, device=cloud.device)
    a = records.ScanTileGatherArgs()
    a.T, a.C, a.max_segments, a.rows = parent.shape[0], cloud.shape[1], max_segments, rows
    a.cloud, a.offset, a.count = cloud.data_ptr(), offset.data_ptr(), count.data_ptr()
    a.parent, a.window, a.base, a.crops = parent.data_ptr(), window.data_ptr(), base.data_ptr(), crops.data_ptr()
    _lib.run("scene_scan_tile_gather", a, cloud.device)
    return crops


def gather_bases(counts):
    """(count (T,) i32, offset (T,) i64, base (T, G) i64) from the (T, G) counts of the built tiles."""
    counts = np.asarray(counts, np.int64)
    count = counts.sum(1)
    offset = scene_offsets(count)
    base = offset[:, None] + np.cumsum(counts, 1) - counts
    return count.astype(np.int32), offset, np.ascontiguousarray(base, np.int64)


# ---------------------------------------------------------------------------------- the store
class TileStore(ScanStore):
    """A ScanStore whose scans are the built tiles of `store`'s scans (`from_store`).  Beyond
    ScanStore's fields: `parent` (T,) the scan of each tile, `first`, `tiles` (S,) each scan's run of
    tiles, `iy`, `ix` (T,) the tile's place in its scan's grid, `window`, `core` (T, 4) float32 (host,
    and in `dev`), `parent_names`, `source` (the parent store), `tile` (tx, ty) and `overlap` as
    given, `reach_dev` (detect_tiled's device tables of its NMS across the cuts, by seam width).
    `clouds` (host rows) and `floor` (host copy) are filled at first use."""

    def __init__(self, *args, **kwargs):
        raise TypeError("TileStore is built by TileStore.from_store(store, tile, overlap, min_points)")

    @classmethod
    def from_store(cls, store, tile, overlap=1.0, min_points=1):
        if isinstance(store, TileStore) or not isinstance(store, ScanStore):
            raise ValueError("TileStore.from_store: a ScanStore (not itself a TileStore)")
        _check_overlap(*_tile_sizes(tile), overlap)  # refused before the first launch
        self = object.__new__(cls)
        self.tile, self.overlap, self.reach_dev = _tile_sizes(tile), float(overlap), {}
        self.source, self.dataset, self.columns = store, store.dataset, store.columns
        self.device, self.dev, self.parent_names = store.device, None, list(store.names)
        self._clouds = self._floor = None
        if store.dev is None:
            grid = tile_grid(host_bounds(store.clouds), tile, overlap, store.names)
            built, self._clouds = host_tiles(store.clouds, grid, min_points)
            self.count = np.array([c.shape[0] for c in self._clouds], np.int32)
            self.offset = scene_offsets(self.count)
            self._grid_fields(grid, built)
            return self
        d = store.dev
        G = _segments(store.count)
        bounds = scan_bounds_gpu(d["cloud"], d["offset"], d["count"], G).cpu().numpy()  # host read 1 of 2
        grid = tile_grid(bounds, tile, overlap, store.names)
        counts = tile_count_gpu(d["cloud"], d["offset"], d["count"], to_device(grid["parent"], self.device),
                                to_device(grid["window"], self.device), G).cpu().numpy()  # host read 2 of 2
        built = select_tiles(grid, counts.sum(1, dtype=np.int64), min_points)
        self._grid_fields(grid, built)
        self.count, self.offset, base = gather_bases(counts[built])
        self.dev = {k: to_device(getattr(self, k), self.device)
                    for k in ("offset", "count", "parent", "window", "core", "first", "tiles", "iy", "ix")}
        self.dev["cloud"] = tile_gather_gpu(d["cloud"], d["offset"], d["count"], self.dev["parent"],
                                            self.dev["window"], to_device(base, self.device),
                                            int(self.count.sum(dtype=np.int64)), G)
        self.dev["floor"], _ = scan_prepare_gpu(self.dev["cloud"], self.dev["offset"], self.dev["count"])
        return self

    def _grid_fields(self, grid, built):
        for k in ("parent", "iy", "ix", "window", "core"):
            setattr(self, k, np.ascontiguousarray(grid[k][built]))
        S = len(self.parent_names)
        self.tiles = np.bincount(self.parent, minlength=S).astype(np.int32)
        self.first = scene_offsets(self.tiles).astype(np.int32)
        self.names = ["%s_tile%02d_%02d" % (self.parent_names[p], y, x)
                      for p, y, x in zip(self.parent, self.iy, self.ix)]

    @property
    def clouds(self):
        if self._clouds is None:
            self._clouds = [self.source.clouds[p][in_box(self.source.clouds[p], w)]
                            for p, w in zip(self.parent, self.window)]
        return self._clouds

    @property
    def floor(self):
        if self._floor is None:
            if self.dev is not None:
                self._floor = self.dev["floor"].cpu().numpy()
            else:
                self._floor = np.array([host_floor(c[:, 2]) for c in self.clouds], np.float32)
        return self._floor
