"""detect(): boxes for scans without labels, from the store to packed detections without the host in
the loop.

    store = ScanStore.from_files(paths, "cuda:0", dataset="scannet")
    loader = ScanLoader(store, 40000)
    found = detect(InferenceEngine(detector), loader, config_dict)
    found[0]["box"], found.by_name("scene0000_00")["corners"], found.as_map_cls(), found.save(out_dir)

Per batch: the loader's launch (scene_scan_batch_build), the engine's pipelined forward
(InferenceEngine.run), for opt_step > 0 iou_opt.optimize_boxes (ordered as inference.evaluate orders
it), parse_predictions_device and ONE more launch, scene_detections_pack (include/scan_hip.h), which
writes each scene's kept proposals compacted and ordered -- objectness probability descending, ties by
proposal index ascending -- into one arena for the whole run.  Nothing in the loop copies to the host
or synchronises; the arena is copied ONCE, when the Detections object is first read.

The arena is a flat float32 buffer of six planes, each indexed by scan (S scans, K proposals, cap = K
rows per scan; the integer planes are stored as their bit patterns):
    count     (S,)        i32   kept proposals of the scan
    proposal  (S, K)      i32   proposal index of each row
    cls       (S, K)      i32   arg-max class
    score     (S, K)      f32   objectness probability; (S, K, C) with per_class_proposal:
                                sem_prob * obj_prob exactly as parse_predictions_device forms it
    box       (S, K, 7)   f32   centre, size (l, w, h), heading in the network's frame
    corners   (S, K, 8, 3) f32  upright camera frame, as parse_predictions returns them
Rows past `count` are zero.  `host_pack` restates the rule in numpy.

detect_tiled() is the same loop over the tiles of a scan_tiles.TileStore and one merge launch into a
second arena, one set of boxes per parent scan (see the section at the end; `host_merge` restates it).
"""
import ctypes
import importlib
import os

import numpy as np
import torch

from .scan_data import ScanLoader, ScanStore

MAX_K = 1024  # SCAN_MAX_K
PLANES = ("count", "proposal", "cls", "score", "box", "corners")

_c_int, _vp = ctypes.c_int, ctypes.c_void_p


class _PackArgs(ctypes.Structure):  # field order == include/scan_hip.h ScanPackArgs
    _fields_ = ([(n, _c_int) for n in ("B", "K", "NC", "scene0")] +
                [(n, _vp) for n in ("keep", "obj_prob", "cls", "score", "center", "size", "heading", "corners",
                                    "count", "proposal", "cls_out", "score_out", "box", "corners_out")])


def arena_layout(S, K, NC):
    """{plane: (first word, shape)} and the arena's size in 4-byte words; NC = 0: one score per row."""
    shapes = {"count": (S,), "proposal": (S, K), "cls": (S, K), "score": (S, K, NC) if NC else (S, K),
              "box": (S, K, 7), "corners": (S, K, 8, 3)}
    layout, at = {}, 0
    for name in PLANES:
        layout[name] = (at, shapes[name])
        at += int(np.prod(shapes[name]))
    return layout, at


def host_pack(keep, obj_prob, cls, score, box, corners):
    """The packing rule in numpy for one batch: keep (B, K) bool, obj_prob (B, K), cls (B, K), score
    (B, K) or (B, K, C), box (B, K, 7), corners (B, K, 8, 3) -> {plane: array} with B leading."""
    keep = np.asarray(keep, bool)
    B, K = keep.shape
    out = {"count": np.zeros(B, np.int32), "proposal": np.zeros((B, K), np.int32), "cls": np.zeros((B, K), np.int32),
           "score": np.zeros(np.shape(score), np.float32), "box": np.zeros((B, K, 7), np.float32),
           "corners": np.zeros((B, K, 8, 3), np.float32)}
    for b in range(B):
        js = np.nonzero(keep[b])[0]
        order = js[np.argsort(-np.asarray(obj_prob[b], np.float32)[js], kind="stable")]
        c = len(order)
        out["count"][b] = c
        out["proposal"][b, :c] = order
        out["cls"][b, :c] = np.asarray(cls[b])[order]
        out["score"][b, :c] = np.asarray(score[b])[order]
        out["box"][b, :c] = np.asarray(box[b])[order]
        out["corners"][b, :c] = np.asarray(corners[b])[order]
    return out


def map_cls_of(rows, num_class, per_class):
    """One scan's packed rows -> the reference's batch_pred_map_cls listing (ap_helper.py:205-219):
    proposals ascending; with per_class every class of every kept box, class-major."""
    c = int(rows["count"])
    by_proposal = np.argsort(rows["proposal"][:c], kind="stable")
    if per_class:
        return [(ii, rows["corners"][r], rows["score"][r, ii]) for ii in range(num_class) for r in by_proposal]
    return [(int(rows["cls"][r]), rows["corners"][r], rows["score"][r]) for r in by_proposal]


def new_arena(S, K, NC, device):
    """The arena of a run of S scans, uninitialised: the pack launches write every word of the rows
    they are given."""
    return torch.empty(arena_layout(S, K, NC)[1], dtype=torch.float32, device=device)


def pack_end_points(arena, S, scene0, end_points, config_dict):
    """parse_predictions_device on one batch's end points and the pack launch into rows [scene0,
    scene0 + B) of the run's arena (arena None: allocated here for S scans) -> (arena, K, NC, B).
    No host copy and no synchronising op."""
    from .eval_helper import decode_boxes, parse_predictions_device
    pred = parse_predictions_device(end_points, config_dict)
    size64, heading64 = decode_boxes(end_points, config_dict['dataset_config'])
    obj_prob = torch.softmax(end_points['objectness_scores'], dim=-1)[:, :, 1]
    B, K = pred['keep'].shape
    NC = pred['score'].shape[2] if config_dict['per_class_proposal'] else 0
    if arena is None:
        arena = new_arena(S, K, NC, pred['keep'].device)
    pack_gpu(arena, S, scene0, pred['keep'], obj_prob, pred['cls'], pred['score'], end_points['center'],
             size64, heading64, pred['corners'])
    return arena, K, NC, B


def pack_gpu(arena, S, scene0, keep, obj_prob, cls, score, center, size64, heading64, corners):
    """Launch scene_detections_pack for one batch into rows [scene0, scene0 + B) of `arena`."""
    _L = importlib.import_module("3dioumatch_amd._lib")
    B, K = keep.shape
    NC = score.shape[2] if score.dim() == 3 else 0
    if K > MAX_K:
        raise ValueError("scene_detections_pack: K = %d proposals, at most %d" % (K, MAX_K))
    layout, words = arena_layout(S, K, NC)
    if arena.dtype != torch.float32 or arena.numel() != words or not arena.is_contiguous():
        raise ValueError("scene_detections_pack: the arena does not match (S, K, C) = (%d, %d, %d)" % (S, K, NC))
    if scene0 < 0 or scene0 + B > S:
        raise ValueError("scene_detections_pack: rows %d..%d outside the arena's %d" % (scene0, scene0 + B, S))
    ins = {"keep": (keep, torch.bool, (B, K)), "obj_prob": (obj_prob, torch.float32, (B, K)),
           "cls": (cls, torch.int64, (B, K)), "score": (score, torch.float32, (B, K, NC) if NC else (B, K)),
           "center": (center, torch.float32, (B, K, 3)), "size": (size64, torch.float64, (B, K, 3)),
           "heading": (heading64, torch.float64, (B, K)), "corners": (corners, torch.float32, (B, K, 8, 3))}
    a = _PackArgs()
    a.B, a.K, a.NC, a.scene0 = B, K, NC, scene0
    held = []
    for name, (t, dtype, shape) in ins.items():
        if t.dtype != dtype or tuple(t.shape) != shape or t.device != arena.device:
            raise ValueError("scene_detections_pack: %s must be %s %s on %s" % (name, dtype, shape, arena.device))
        t = t.contiguous()
        held.append(t)
        setattr(a, name, t.data_ptr())
    base = arena.data_ptr()
    for plane, field in zip(PLANES, ("count", "proposal", "cls_out", "score_out", "box", "corners_out")):
        setattr(a, field, base + 4 * layout[plane][0])
    with torch.cuda.device(arena.device):
        _L.check(_L.lib.scene_detections_pack(ctypes.byref(a), _L.current_stream_ptr(arena.device)),
                 "scene_detections_pack")
    return arena


class Detections(object):
    """The packed detections of a run.  Reading (indexing, by_name, as_map_cls, save) makes the one
    device -> host copy of the arena; `arena` itself stays on the device."""
    INT_PLANES = ("count", "proposal", "cls")  # stored as their bit patterns

    def __init__(self, arena, names, K, NC, num_class):
        self.arena, self.names, self.K, self.NC, self.num_class = arena, list(names), int(K), int(NC), int(num_class)
        self.per_class_proposal = NC > 0
        self.layout, _ = arena_layout(len(self.names), self.K, self.NC)
        self._planes = None

    def __len__(self):
        return len(self.names)

    def planes(self):
        """{plane: numpy view with the scans leading} of the host copy."""
        if self._planes is None:
            host = self.arena.cpu().numpy() if torch.is_tensor(self.arena) else np.asarray(self.arena, np.float32)
            self._planes = {}
            for name, (at, shape) in self.layout.items():
                flat = host[at:at + int(np.prod(shape))]
                if name in self.INT_PLANES:
                    flat = flat.view(np.int32)
                self._planes[name] = flat.reshape(shape)
        return self._planes

    def __getitem__(self, i):
        i = int(i)
        if not -len(self) <= i < len(self):
            raise IndexError(i)
        return {name: p[i] for name, p in self.planes().items()}

    def by_name(self, name):
        return self[self.names.index(name)]

    def as_map_cls(self):
        """Per scan the listing parse_predictions gives for the same end points."""
        return [map_cls_of(self[i], self.num_class, self.per_class_proposal) for i in range(len(self))]

    def save(self, directory):
        """<name>.npz per scan: count, and the planes cut to the scan's `count` rows."""
        os.makedirs(directory, exist_ok=True)
        for i, name in enumerate(self.names):
            rows = self[i]
            c = int(rows["count"])
            np.savez(os.path.join(directory, name + ".npz"), count=rows["count"],
                     **{k: v[:c] for k, v in rows.items() if k != "count"})


def _pack_run(who, engine, store_or_loader, config_dict, batch_size, opt_step, opt_rate, counter):
    """The loop of detect() and detect_tiled(): every scan of the loader's store through the engine
    and the pack launch -> (store, arena, K, NC).  Nothing in it copies to the host or synchronises."""
    from .iou_opt import _check_detector, optimize_boxes
    loader = store_or_loader
    if isinstance(loader, ScanStore):
        loader = ScanLoader(loader, 40000 if loader.dataset == "scannet" else 20000)
    if not isinstance(loader, ScanLoader):
        raise ValueError("%s: a ScanStore or a ScanLoader" % who)
    store = loader.store
    if store.device is None or store.device != engine.device:
        raise ValueError("%s: the store lives on %s, the engine on %s" % (who, store.device, engine.device))
    if not 1 <= batch_size <= 64:
        raise ValueError("%s: batch_size 1..64" % who)
    detector = engine.detector
    if detector.training:
        raise ValueError("%s: the detector must be in eval mode" % who)
    if opt_step > 0:
        _check_detector(detector)
    S = len(store)
    clouds = []  # the batches engine.run has drawn and not yet returned

    def feed():
        for b in loader.batches(batch_size, counter):
            clouds.append(b['point_clouds'])
            yield b['point_clouds']

    arena, scene0, K, NC = None, 0, 0, 0
    with torch.cuda.device(engine.device):
        for end_points in engine.run(feed()):
            point_clouds = clouds.pop(0)
            if opt_step > 0:
                end_points = optimize_boxes(detector, end_points, opt_rate, opt_step)
            end_points.setdefault('point_clouds', point_clouds)
            arena, K, NC, B = pack_end_points(arena, S, scene0, end_points, config_dict)
            scene0 += B
    return store, arena, K, NC


@torch.no_grad()
def detect(engine, store_or_loader, config_dict, batch_size=8, opt_step=0, opt_rate=5e-4, counter=0):
    """Detections of every scan of a ScanLoader (or of a ScanStore, through ScanLoader(store, 40000
    points for ScanNet / 20000 for SUN RGB-D, height only)), batch_size scans at a time, batch i drawn
    with counter + i.  `engine`: an InferenceEngine; `config_dict`: parse_predictions' keys."""
    store, arena, K, NC = _pack_run("detect", engine, store_or_loader, config_dict, batch_size, opt_step, opt_rate,
                                    counter)
    return Detections(arena, store.names, K, NC, config_dict['dataset_config'].num_class)


# ------------------------------------------------------------------ scans larger than a room
# The tiles of a scan_tiles.TileStore go through the loop above like any scans; ONE more launch,
# scene_detections_merge (include/scan_tile_hip.h), then writes for every parent scan the rows its
# tiles OWN -- those whose box centre (x, y) lies in the tile's core, float32 compares, lower bound
# inclusive -- compacted into a second arena: the scan's tiles in store order, each tile's rows in
# their packed order.  Its planes, indexed by parent scan (cap = (most tiles any scan has) * K rows per
# scan):
#     count (S,), tile (S, cap) i32: the row's tile (its row in the tile store), proposal, cls (S, cap),
#     score (S, cap) or (S, cap, NC), box (S, cap, 7), corners (S, cap, 8, 3)
# Rows past `count` are zero.  There is no cross-tile NMS: a box whose centre two neighbouring tiles
# estimate on opposite sides of a cut may be kept twice or not at all.
MERGED_PLANES = ("count", "tile", "proposal", "cls", "score", "box", "corners")


class _MergeArgs(ctypes.Structure):  # field order == include/scan_tile_hip.h ScanMergeArgs
    _fields_ = ([(n, _c_int) for n in ("S", "K", "NC", "cap", "max_tiles")] +
                [(n, _vp) for n in ("first", "tiles", "core", "count_in", "proposal_in", "cls_in", "score_in",
                                    "box_in", "corners_in", "count", "tile", "proposal", "cls", "score", "box",
                                    "corners")])


def merged_layout(S, cap, NC):
    """arena_layout for the merged arena: {plane: (first word, shape)} and its size in words."""
    shapes = {"count": (S,), "tile": (S, cap), "proposal": (S, cap), "cls": (S, cap),
              "score": (S, cap, NC) if NC else (S, cap), "box": (S, cap, 7), "corners": (S, cap, 8, 3)}
    layout, at = {}, 0
    for name in MERGED_PLANES:
        layout[name] = (at, shapes[name])
        at += int(np.prod(shapes[name]))
    return layout, at


def host_merge(planes, first, tiles, core, cap=None):
    """The merge rule in numpy: `planes` = the tile arena's {plane: array} with the tiles leading
    (Detections.planes()), first / tiles (S,) each scan's run of tiles, core (T, 4) = clo_x, chi_x,
    clo_y, chi_y -> the merged {plane: array} with the scans leading."""
    first, tiles = np.asarray(first, np.int64), np.asarray(tiles, np.int64)
    core = np.asarray(core, np.float32)
    S, K = len(first), planes["proposal"].shape[1]
    if cap is None:
        cap = int(tiles.max()) * K
    out = {"count": np.zeros(S, np.int32), "tile": np.zeros((S, cap), np.int32)}
    for name in ("proposal", "cls", "score", "box", "corners"):
        out[name] = np.zeros((S, cap) + planes[name].shape[2:], planes[name].dtype)
    for s in range(S):
        at = 0
        for t in range(first[s], first[s] + tiles[s]):
            c = int(planes["count"][t])
            xy = np.asarray(planes["box"][t, :c, 0:2], np.float32)
            lo_x, hi_x, lo_y, hi_y = core[t]
            owned = np.nonzero((lo_x <= xy[:, 0]) & (xy[:, 0] < hi_x) & (lo_y <= xy[:, 1]) & (xy[:, 1] < hi_y))[0]
            n = len(owned)
            out["tile"][s, at:at + n] = t
            for name in ("proposal", "cls", "score", "box", "corners"):
                out[name][s, at:at + n] = planes[name][t, owned]
            at += n
        out["count"][s] = at
    return out


def new_merged_arena(S, cap, NC, device):
    """The merged arena of S scans, uninitialised: the merge launch writes every word."""
    return torch.empty(merged_layout(S, cap, NC)[1], dtype=torch.float32, device=device)


def merge_gpu(merged, tile_arena, first, tiles, core, S, T, K, NC, cap, max_tiles):
    """Launch scene_detections_merge: the tile arena (T tiles, K rows each) -> `merged` (S scans, cap
    rows each); first, tiles (S,) int32 and core (T, 4) float32 on the arenas' device."""
    _L = importlib.import_module("3dioumatch_amd._lib")
    if K > MAX_K:
        raise ValueError("scene_detections_merge: K = %d rows per tile, at most %d" % (K, MAX_K))
    if cap < max_tiles * K:
        raise ValueError("scene_detections_merge: cap = %d rows per scan, %d tiles of %d need %d"
                         % (cap, max_tiles, K, max_tiles * K))
    lin, words_in = arena_layout(T, K, NC)
    lout, words_out = merged_layout(S, cap, NC)
    for name, t, words in (("tile arena", tile_arena, words_in), ("merged arena", merged, words_out)):
        if t.dtype != torch.float32 or t.numel() != words or not t.is_contiguous() or t.device != merged.device:
            raise ValueError("scene_detections_merge: the %s does not match (S, T, K, C, cap) = (%d, %d, %d, %d, %d)"
                             % (name, S, T, K, NC, cap))
    for name, t, dtype, shape in (("first", first, torch.int32, (S,)), ("tiles", tiles, torch.int32, (S,)),
                                  ("core", core, torch.float32, (T, 4))):
        if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != merged.device:
            raise ValueError("scene_detections_merge: %s must be %s %s on %s" % (name, dtype, shape, merged.device))
    a = _MergeArgs()
    a.S, a.K, a.NC, a.cap, a.max_tiles = S, K, NC, cap, max_tiles
    a.first, a.tiles, a.core = first.data_ptr(), tiles.data_ptr(), core.data_ptr()
    for plane in PLANES:
        setattr(a, plane + "_in", tile_arena.data_ptr() + 4 * lin[plane][0])
    for plane in MERGED_PLANES:
        setattr(a, plane, merged.data_ptr() + 4 * lout[plane][0])
    with torch.cuda.device(merged.device):
        _L.check(_L.lib.scene_detections_merge(ctypes.byref(a), _L.current_stream_ptr(merged.device)),
                 "scene_detections_merge")
    return merged


def merged_map_cls_of(rows, num_class, per_class):
    """map_cls_of for a scan's merged rows: tile, then proposal ascending; with per_class class-major."""
    c = int(rows["count"])
    order = np.lexsort((rows["proposal"][:c], rows["tile"][:c]))
    if per_class:
        return [(ii, rows["corners"][r], rows["score"][r, ii]) for ii in range(num_class) for r in order]
    return [(int(rows["cls"][r]), rows["corners"][r], rows["score"][r]) for r in order]


class TiledDetections(Detections):
    """The merged detections of a detect_tiled run, one set per PARENT scan, over the merged layout;
    `tiles` is the Detections of the tiles themselves (the first arena) and `store` the TileStore.
    Reading makes the one device -> host copy of the merged arena."""
    INT_PLANES = Detections.INT_PLANES + ("tile",)

    def __init__(self, arena, store, cap, K, NC, num_class, tiles=None):
        self.arena, self.names, self.K, self.NC, self.num_class = arena, list(store.parent_names), int(K), int(NC), \
            int(num_class)
        self.store, self.cap, self.tiles = store, int(cap), tiles
        self.per_class_proposal = NC > 0
        self.layout, _ = merged_layout(len(self.names), self.cap, self.NC)
        self._planes = None

    def as_map_cls(self):
        return [merged_map_cls_of(self[i], self.num_class, self.per_class_proposal) for i in range(len(self))]

    def save(self, directory):
        """<scan>.npz per parent scan: count, the planes cut to `count` rows (`tile` among them: rows of
        the tile store), and of the scan's tiles `tile_first` (the store row of its first tile),
        `tile_names`, `window` and `core` (tiles, 4)."""
        os.makedirs(directory, exist_ok=True)
        st = self.store
        for i, name in enumerate(self.names):
            rows = self[i]
            c = int(rows["count"])
            a, b = int(st.first[i]), int(st.first[i] + st.tiles[i])
            np.savez(os.path.join(directory, name + ".npz"), count=rows["count"], tile_first=np.int32(a),
                     tile_names=np.array(st.names[a:b]), window=st.window[a:b], core=st.core[a:b],
                     **{k: v[:c] for k, v in rows.items() if k != "count"})


@torch.no_grad()
def detect_tiled(engine, tile_store_or_loader, config_dict, batch_size=8, opt_step=0, opt_rate=5e-4, counter=0):
    """detect() for scans larger than a room: the tiles of a scan_tiles.TileStore (or of a ScanLoader
    over one) through detect()'s loop, then ONE merge launch -> TiledDetections, one set per parent
    scan in the scan's own frame.  No host copy and no synchronising op before the result is read."""
    from .scan_tiles import TileStore
    loader = tile_store_or_loader
    store = loader.store if isinstance(loader, ScanLoader) else loader
    if not isinstance(store, TileStore):
        raise ValueError("detect_tiled: a TileStore or a ScanLoader over one")
    store, arena, K, NC = _pack_run("detect_tiled", engine, loader, config_dict, batch_size, opt_step, opt_rate,
                                    counter)
    S, T = len(store.parent_names), len(store)
    max_tiles = int(store.tiles.max())
    cap = max_tiles * K
    with torch.cuda.device(engine.device):
        merged = new_merged_arena(S, cap, NC, arena.device)
        merge_gpu(merged, arena, store.dev["first"], store.dev["tiles"], store.dev["core"], S, T, K, NC, cap,
                  max_tiles)
    num_class = config_dict['dataset_config'].num_class
    return TiledDetections(merged, store, cap, K, NC, num_class, Detections(arena, store.names, K, NC, num_class))
