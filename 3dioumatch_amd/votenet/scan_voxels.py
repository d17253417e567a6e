"""Voxel-grid downsampling of scan stores on the device: one row per occupied cell.

    big = ScanStore.from_files(paths, "cuda:0")               # registered scans: dense where they overlap
    even = VoxelStore.from_store(big, voxel=0.05)              # one row per 5 cm cell, still resident
    tiles = TileStore.from_store(even, tile=(8.0, 8.0))        # ... and on as before

Where two registered scans overlap a cloud is twice as dense, next to the scanner a hundred times;
`ScanLoader` draws uniformly over ROWS, so its sample sits where the rows are.  `VoxelStore` is a
`ScanStore` that keeps one row per occupied cell of a grid (`ScanLoader`, `detect`, `TileStore.from_store`
and `detect_tiled` take it unchanged) and remembers where each kept row came from.

Semantics (float64 on both sides: the numpy restatement is bit-exact).  `voxel` is one size or three
(vx, vy, vz) in metres, finite and > 0.  The cell of a row p is c_a = floor(float64(p_a) / v_a) per axis:
the grid is absolute, anchored at the origin, so a point falls into the same cell in every scan and
tile; -0.0 and +0.0 are cell 0; a coordinate on a face belongs to the upper cell.  A scan with a cell
|c_a| >= 2^20 is refused (ValueError naming it).  The cell's key is the 63-bit word
((c_z + 2^20) << 42) | ((c_y + 2^20) << 21) | (c_x + 2^20).  A cell keeps its row with the smallest rank:
    keep="first"    the row's index in its scan: the cell's earliest row;
    keep="nearest"  (bits(float32(d2)) << 32) | index with d_a = float64(p_a) - (c_a + 0.5) v_a and
                    d2 = (d_x d_x + d_y d_y) + d_z d_z in float64, rounded once to float32: the row closest
                    to the cell's centre, ties to the lowest index.
The kept rows come in the scan's own order, all columns bit for bit; `source` gives each kept row's
index in its parent scan.  Scans never interact.

Construction on the device (include/scan_voxel_hip.h): scene_scan_voxel_mark (clear, then one thread
per row into a per-scan open-addressing table: compare-and-swap on the key, minimum of the rank),
scene_scan_voxel_count; the host reads the (S, segments) counts and the S out-of-range counters in one
copy -- the only read -- refuses or forms every output row; scene_scan_voxel_gather writes the rows and
`source` (TileStore's stable compaction); scene_scan_prepare gives every result its own floor.  Which
thread claims a slot of the table varies; the key set and each cell's minimum do not, so two
constructions are bit-equal.  `host_voxels` is the numpy restatement and the path of a `device=None`
parent.

Left out: a centroid mode (a deterministic float mean needs an ordered sum), the inverse map from a
parent row to its kept row, and a table sized by occupancy (it is sized for load 0.5 whatever the
scan's redundancy).
"""
import numpy as np
import torch

from .. import records
from .scan_data import ScanStore, host_floor, scan_prepare_gpu
from .scan_tiles import TileStore, _segments, gather_bases
from .scene_loader import scene_offsets, to_device

CELL_LIMIT = 1 << 20  # SCAN_VOXEL_CELL_LIMIT
KEEP = ("first", "nearest")


# ---------------------------------------------------------------------------------- the grid
def voxel_sizes(voxel):
    """(vx, vy, vz) float64 from one size or three, each finite and > 0."""
    try:
        v = np.asarray(voxel, np.float64).reshape(-1)
    except (TypeError, ValueError):
        v = np.zeros(0)
    if v.shape[0] == 1:
        v = np.repeat(v, 3)
    if v.shape[0] != 3 or not np.isfinite(v).all() or (v <= 0).any():
        raise ValueError("voxel: one or three sizes in metres, each finite and > 0, got %r" % (voxel,))
    return float(v[0]), float(v[1]), float(v[2])


def _keep(keep):
    if keep not in KEEP:
        raise ValueError("keep must be one of %s, got %r" % (KEEP, keep))
    return keep


def voxel_cells(cloud, voxel):
    """(n, 3) int64: the cell of every row of a float32 cloud, floor(float64(p) / v) per axis."""
    p = np.asarray(cloud, np.float32)[:, 0:3].astype(np.float64)
    return np.floor(p / np.array(voxel_sizes(voxel))).astype(np.int64)


def voxel_keys(cells):
    """(n,) int64 keys of (n, 3) cells with |c| < 2^20; ValueError for a cell out of range."""
    c = np.asarray(cells, np.int64).reshape(-1, 3)
    if (np.abs(c) >= CELL_LIMIT).any():
        raise ValueError("cells out of range: |c| < 2^20")
    c = c + CELL_LIMIT
    return (c[:, 2] << 42) | (c[:, 1] << 21) | c[:, 0]


def voxel_ranks(cloud, cells, voxel, keep):
    """(n,) uint64: the rank word of every row (module docstring)."""
    n = len(cells)
    index = np.arange(n, dtype=np.uint64)
    if _keep(keep) == "first":
        return index
    v = np.array(voxel_sizes(voxel))
    p = np.asarray(cloud, np.float32)[:, 0:3].astype(np.float64)
    d = p - (np.asarray(cells, np.int64).astype(np.float64) + 0.5) * v
    d2 = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(np.float32)
    return (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | index


def host_voxels(clouds, voxel, keep="first", names=None):
    """numpy restatement of the construction: per scan the indices (int32, ascending) of the rows
    that are kept.  ValueError naming the scans that have a cell out of range."""
    sizes, keep = voxel_sizes(voxel), _keep(keep)
    cells = [voxel_cells(c, sizes) for c in clouds]
    _refuse([int((np.abs(c) >= CELL_LIMIT).any(1).sum()) for c in cells], names, sizes)
    kept = []
    for cloud, c in zip(clouds, cells):
        keys, ranks = voxel_keys(c), voxel_ranks(cloud, c, sizes, keep)
        order = np.lexsort((ranks, keys))  # by key, then rank: the first of every key's run is kept
        head = np.ones(len(order), bool)
        head[1:] = keys[order][1:] != keys[order][:-1]
        kept.append(np.sort(order[head]).astype(np.int32))
    return kept


def _refuse(outside, names, sizes):
    bad = ["%s (%d)" % (names[i] if names is not None else "scan %d" % i, n) for i, n in enumerate(outside) if n]
    if bad:
        raise ValueError("scans with points beyond 2^20 cells of %g m x %g m x %g m from the origin (count): %s"
                         % (sizes + (", ".join(bad),)))


# ---------------------------------------------------------------------------------- the launches
def voxel_slots(count):
    """scene_scan_voxel_slots: the table slots of a scan of `count` rows."""
    count = int(count)
    if count < 1 or count >= 1 << 30:
        return 0
    return max(2, 1 << (2 * count - 1).bit_length())


def _mark_record(cloud, offset, count, sizes, keep, mark, max_segments):
    a = records.ScanVoxelArgs()
    a.S, a.C, a.max_segments, a.nearest = count.shape[0], cloud.shape[1], max_segments, int(_keep(keep) == "nearest")
    a.voxel[0], a.voxel[1], a.voxel[2] = sizes
    a.total_slots = mark["total_slots"]
    a.scratch_bytes = mark["scratch"].numel() * mark["scratch"].element_size()
    a.cloud, a.offset, a.count = cloud.data_ptr(), offset.data_ptr(), count.data_ptr()
    a.slot_offset, a.scratch = mark["slot_offset"].data_ptr(), mark["scratch"].data_ptr()
    a.slot, a.outside = mark["slot"].data_ptr(), mark["outside"].data_ptr()
    return a


def voxel_mark_gpu(cloud, offset, count, host_count, voxel, keep, max_segments, scratch=None, slot=None, table=None):
    """The marking launches (clear, insert) over the scans of a flat (P, C) device cloud; `host_count`
    is the host copy of `count`, from which the table's runs are laid out.  Returns the mark: a dict of
    `scratch` (2 * total_slots int64: key words, best words), `slot` (P,) int32, `table`
    (S * max_segments + S,) int32 -- scene_scan_voxel_count's counts followed by the S out-of-range
    counters, one buffer so that the host reads both in one copy -- its tail `outside`, `slot_offset`
    (S,) int64 and `total_slots`.  `scratch`, `slot` and `table` may be given; they may hold anything."""
    from .. import _lib
    sizes, S, dev = voxel_sizes(voxel), count.shape[0], cloud.device
    slots = np.array([voxel_slots(n) for n in host_count], np.int64)
    total = int(slots.sum())
    if scratch is None:
        scratch = torch.empty(2 * total, dtype=torch.int64, device=dev)
    if slot is None:
        slot = torch.empty(cloud.shape[0], dtype=torch.int32, device=dev)
    if table is None:
        table = torch.empty(S * max_segments + S, dtype=torch.int32, device=dev)
    mark = {"scratch": scratch, "slot": slot, "table": table, "outside": table[S * max_segments:],
            "slot_offset": to_device(scene_offsets(slots), dev), "total_slots": total}
    _lib.run("scene_scan_voxel_mark", _mark_record(cloud, offset, count, sizes, keep, mark, max_segments), dev)
    return mark


def voxel_count_gpu(cloud, offset, count, voxel, keep, mark, max_segments):
    """(S, max_segments) int32, a view of the mark's table: per scan and segment the rows that are kept."""
    from .. import _lib
    S = count.shape[0]
    counts = mark["table"][:S * max_segments].view(S, max_segments)
    a = records.ScanVoxelCountArgs()
    a.mark = _mark_record(cloud, offset, count, voxel_sizes(voxel), keep, mark, max_segments)
    a.counts = counts.data_ptr()
    _lib.run("scene_scan_voxel_count", a, cloud.device)
    return counts


def voxel_gather_gpu(cloud, offset, count, voxel, keep, mark, base, rows, max_segments, out=None, source=None):
    """((rows, C) float32, (rows,) int32): the kept rows, segment g of scan s written from row
    base[s, g] on, and each one's index in its scan.  `out` and `source` may be given."""
    from .. import _lib
    if out is None:
        out = torch.empty((rows, cloud.shape[1]), dtype=torch.float32, device=cloud.device)
    if source is None:
        source = torch.empty((rows,), dtype=torch.int32, device=cloud.device)
    a = records.ScanVoxelGatherArgs()
    a.mark = _mark_record(cloud, offset, count, voxel_sizes(voxel), keep, mark, max_segments)
    a.rows, a.base, a.out, a.source = rows, base.data_ptr(), out.data_ptr(), source.data_ptr()
    _lib.run("scene_scan_voxel_gather", a, cloud.device)
    return out, source


# ---------------------------------------------------------------------------------- the store
class VoxelStore(ScanStore):
    """A ScanStore of `store`'s scans, each downsampled to one row per occupied cell (`from_store`).
    Beyond ScanStore's fields: `source_store` (the parent store), `voxel` (vx, vy, vz) and `keep` as
    given, `source` (rows,) int32, each kept row's index in its parent scan (flat, by `offset`; in
    `dev` too).  The names are the parent's.  `clouds` (host rows), `floor` and `source` (host
    copies) are filled at first use."""

    def __init__(self, *args, **kwargs):
        raise TypeError("VoxelStore is built by VoxelStore.from_store(store, voxel, keep)")

    @classmethod
    def from_store(cls, store, voxel, keep="first"):
        if isinstance(store, TileStore) or not isinstance(store, ScanStore):
            raise ValueError("VoxelStore.from_store: a ScanStore that is not a TileStore (downsample, then tile)")
        sizes, keep = voxel_sizes(voxel), _keep(keep)  # refused before the first launch
        self = object.__new__(cls)
        self.source_store, self.voxel, self.keep = store, sizes, keep
        self.dataset, self.columns, self.names = store.dataset, store.columns, list(store.names)
        self.device, self.dev = store.device, None
        self._clouds = self._floor = self._source = None
        if store.dev is None:
            kept = host_voxels(store.clouds, sizes, keep, store.names)
            self.count = np.array([len(k) for k in kept], np.int32)
            self.offset = scene_offsets(self.count)
            self._source = np.concatenate(kept).astype(np.int32)
            return self
        d = store.dev
        S, G = len(store.count), _segments(store.count)
        mark = voxel_mark_gpu(d["cloud"], d["offset"], d["count"], store.count, sizes, keep, G)
        voxel_count_gpu(d["cloud"], d["offset"], d["count"], sizes, keep, mark, G)
        table = mark["table"].cpu().numpy()  # the one host read
        _refuse(table[S * G:], store.names, sizes)
        self.count, self.offset, base = gather_bases(table[:S * G].reshape(S, G))
        self.dev = {"offset": to_device(self.offset, self.device), "count": to_device(self.count, self.device)}
        self.dev["cloud"], self.dev["source"] = voxel_gather_gpu(
            d["cloud"], d["offset"], d["count"], sizes, keep, mark, to_device(base, self.device),
            int(self.count.sum(dtype=np.int64)), G)
        self.dev["floor"], _ = scan_prepare_gpu(self.dev["cloud"], self.dev["offset"], self.dev["count"])
        return self

    @property
    def source(self):
        if self._source is None:
            self._source = self.dev["source"].cpu().numpy()
        return self._source

    @property
    def clouds(self):
        if self._clouds is None:
            src = self.source
            self._clouds = [self.source_store.clouds[s][src[o:o + c]]
                            for s, (o, c) in enumerate(zip(self.offset, self.count))]
        return self._clouds

    @property
    def floor(self):
        if self._floor is None:
            if self.dev is not None:
                self._floor = self.dev["floor"].cpu().numpy()
            else:
                self._floor = np.array([host_floor(c[:, 2]) for c in self.clouds], np.float32)
        return self._floor
