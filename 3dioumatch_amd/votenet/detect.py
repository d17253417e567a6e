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
With seam_nms=True that merge is an NMS across the cuts, one box per object that two tiles see
(scene_detections_merge_nms, four launches; the last section; `host_merge_nms` restates it).
"""
import os

import numpy as np
import torch

from .. import records
from .scan_data import ScanLoader, ScanStore

MAX_K = 1024  # SCAN_MAX_K
PLANES = ("count", "proposal", "cls", "score", "box", "corners")


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
    from .. import _lib
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
    a = records.ScanPackArgs()
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
    _lib.run("scene_detections_pack", a, arena.device)
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
# Rows past `count` are zero.  This merge has no cross-tile NMS: a box whose centre two neighbouring
# tiles estimate on opposite sides of a cut may be kept twice or not at all (seam_nms, further down, is
# the merge that has one).
MERGED_PLANES = ("count", "tile", "proposal", "cls", "score", "box", "corners")


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
    from .. import _lib
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
    a = records.ScanMergeArgs()
    a.S, a.K, a.NC, a.cap, a.max_tiles = S, K, NC, cap, max_tiles
    a.first, a.tiles, a.core = first.data_ptr(), tiles.data_ptr(), core.data_ptr()
    for plane in PLANES:
        setattr(a, plane + "_in", tile_arena.data_ptr() + 4 * lin[plane][0])
    for plane in MERGED_PLANES:
        setattr(a, plane, merged.data_ptr() + 4 * lout[plane][0])
    _lib.run("scene_detections_merge", a, merged.device)
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
    `seam` is None for the plain merge, else the settings of the NMS across the cuts (seam, thresh,
    old_type, same_class, dims) and `reach` its (T, 4) table.  Reading makes the one device -> host
    copy of the merged arena."""
    INT_PLANES = Detections.INT_PLANES + ("tile",)

    def __init__(self, arena, store, cap, K, NC, num_class, tiles=None, seam=None, reach=None):
        self.arena, self.names, self.K, self.NC, self.num_class = arena, list(store.parent_names), int(K), int(NC), \
            int(num_class)
        self.store, self.cap, self.tiles = store, int(cap), tiles
        self.seam, self.reach = seam, reach
        self.per_class_proposal = NC > 0
        self.layout, _ = merged_layout(len(self.names), self.cap, self.NC)
        self._planes = None

    def as_map_cls(self):
        return [merged_map_cls_of(self[i], self.num_class, self.per_class_proposal) for i in range(len(self))]

    def save(self, directory):
        """<scan>.npz per parent scan: count, the planes cut to `count` rows (`tile` among them: rows of
        the tile store), and of the scan's tiles `tile_first` (the store row of its first tile),
        `tile_names`, `window` and `core` (tiles, 4); after an NMS across the cuts also `seam`,
        `seam_thresh`, `seam_old_type`, `seam_same_class`, `seam_dims` and `reach` (tiles, 4)."""
        os.makedirs(directory, exist_ok=True)
        st = self.store
        for i, name in enumerate(self.names):
            rows = self[i]
            c = int(rows["count"])
            a, b = int(st.first[i]), int(st.first[i] + st.tiles[i])
            extra = {}
            if self.seam is not None:
                extra = {"seam": np.float64(self.seam["seam"]), "seam_thresh": np.float64(self.seam["thresh"]),
                         "seam_old_type": np.int32(self.seam["old_type"]),
                         "seam_same_class": np.int32(self.seam["same_class"]),
                         "seam_dims": np.int32(self.seam["dims"]), "reach": self.reach[a:b]}
            np.savez(os.path.join(directory, name + ".npz"), count=rows["count"], tile_first=np.int32(a),
                     tile_names=np.array(st.names[a:b]), window=st.window[a:b], core=st.core[a:b],
                     **extra, **{k: v[:c] for k, v in rows.items() if k != "count"})


@torch.no_grad()
def detect_tiled(engine, tile_store_or_loader, config_dict, batch_size=8, opt_step=0, opt_rate=5e-4, counter=0,
                 seam_nms=False, seam=None):
    """detect() for scans larger than a room: the tiles of a scan_tiles.TileStore (or of a ScanLoader
    over one) through detect()'s loop, then ONE merge launch -> TiledDetections, one set per parent
    scan in the scan's own frame.  No host copy and no synchronising op before the result is read.

    seam_nms: merge with an NMS across the cuts instead (scene_detections_merge_nms, four launches;
    the section below) over the rows whose centre lies within `seam` metres of their tile's core;
    seam None: the store's overlap / 2.  The settings are config_dict's nms_iou, use_old_type_nms,
    use_3d_nms and cls_nms (seam_settings)."""
    from .scan_tiles import TileStore
    loader = tile_store_or_loader
    store = loader.store if isinstance(loader, ScanLoader) else loader
    if not isinstance(store, TileStore):
        raise ValueError("detect_tiled: a TileStore or a ScanLoader over one")
    if seam is not None and not seam_nms:
        raise ValueError("detect_tiled: seam = %r without seam_nms" % (seam,))
    settings = reach = None
    if seam_nms:
        settings = seam_settings(config_dict, store.overlap / 2 if seam is None else seam)
        reach = seam_reach(store.core, settings["seam"])  # refused before the first launch
    store, arena, K, NC = _pack_run("detect_tiled", engine, loader, config_dict, batch_size, opt_step, opt_rate,
                                    counter)
    S, T = len(store.parent_names), len(store)
    max_tiles = int(store.tiles.max())
    cap = max_tiles * K
    d = store.dev
    with torch.cuda.device(engine.device):
        merged = new_merged_arena(S, cap, NC, arena.device)
        if seam_nms:
            if settings["seam"] not in store.reach_dev:  # one upload per seam width
                store.reach_dev[settings["seam"]] = torch.from_numpy(reach).to(arena.device)
            merge_nms_gpu(merged, arena, d["first"], d["tiles"], d["core"], d["iy"], d["ix"],
                          store.reach_dev[settings["seam"]], S, T, K, NC, cap, max_tiles, settings["thresh"],
                          settings["old_type"], settings["same_class"], settings["dims"])
        else:
            merge_gpu(merged, arena, d["first"], d["tiles"], d["core"], S, T, K, NC, cap, max_tiles)
    num_class = config_dict['dataset_config'].num_class
    return TiledDetections(merged, store, cap, K, NC, num_class, Detections(arena, store.names, K, NC, num_class),
                           seam=settings, reach=reach)


# ------------------------------------------------------------------ an NMS across the cuts
# Each tile estimates the centre of an object near a cut on its own, so the plain merge may keep the
# object twice (both tiles put the centre on their own side) or not at all (each puts it on the
# other's).  scene_detections_merge_nms (include/scan_tile_hip.h) therefore looks past the core:
#   reach      the core grown by `seam` metres on every finite side; float64 on the host, rounded once.
#   candidate  a packed row whose centre lies in its tile's reach; OWNED if it lies in the core, else
#              a GUEST.
#   bounds     min / max of the row's eight packed corners per axis (float32, camera frame: what
#              nms_3d_faster sees); area / volume, intersection and overlap in float64 in the
#              expression order of nms_aabb_block_kernel; dims 2: the camera x / z footprint.
#   key        score[row], or score[row, cls[row]] with per-class scores; the order is key
#              descending, then tile, then packed row ascending.
#   partners   two candidates of different, neighbouring tiles of one scan (|iy - iy'| <= 1 and
#              |ix - ix'| <= 1) whose overlap is > thresh.  Rows of one tile never interact: the
#              per-tile NMS has judged them.
#   winner     in that order, a candidate none of whose higher-ordered partners is a winner.
#   kept       an owned winner; a guest that is a winner AND has a partner.  An unmatched guest is
#              dropped, so where no two tiles' boxes overlap the result is the plain merge.
# The output is the merged layout above, the kept rows in tile order and packed order.
def seam_settings(config_dict, seam):
    """{seam, thresh, old_type, same_class, dims} of the NMS across the cuts from parse_predictions'
    keys: nms_iou, use_old_type_nms, dims 3 with use_3d_nms else 2, and cls_nms in 3-D only, as
    parse_predictions_device applies them.  use_iou_for_nms is NOT consulted: the key is the packed
    score, whatever the per-tile NMS ranked by."""
    dims = 3 if config_dict['use_3d_nms'] else 2
    return {"seam": float(seam), "thresh": float(config_dict['nms_iou']),
            "old_type": int(bool(config_dict['use_old_type_nms'])),
            "same_class": int(bool(config_dict['cls_nms']) and dims == 3), "dims": dims}


def seam_reach(core, seam):
    """(T, 4) float32 rlo_x, rhi_x, rlo_y, rhi_y: clo - seam, chi + seam in float64 from the float32
    core, rounded once to float32; an infinite side stays infinite.  0 <= seam < inf."""
    seam = float(seam)
    if not 0 <= seam < np.inf:
        raise ValueError("seam = %r metres: 0 <= seam" % (seam,))
    core = np.asarray(core, np.float32).reshape(-1, 4).astype(np.float64)
    reach = np.stack([core[:, 0] - seam, core[:, 1] + seam, core[:, 2] - seam, core[:, 3] + seam], 1)
    return np.ascontiguousarray(reach.astype(np.float32))


def host_merge_nms(planes, first, tiles, core, iy, ix, reach, thresh, old_type, same_class, dims, cap=None,
                   info=None):
    """The rule of the NMS across the cuts in numpy (the comment above), host_merge's arguments plus
    iy, ix (T,), reach (T, 4) and the four settings -> the merged {plane: array}.  A sort and a loop
    over the pairs in its order.  `info`, a dict, receives per scan `pairs` (partner pairs), `rounds`
    (the longest chain of decisions that wait on one another), `kept_guests`, `dropped_owned`,
    `most_candidates` (of one tile) and `most_above` (higher-ordered partners of one row)."""
    if dims not in (2, 3) or (dims == 2 and same_class):
        raise ValueError("host_merge_nms: dims 2 or 3, same_class with 3 only")
    first, tiles = np.asarray(first, np.int64), np.asarray(tiles, np.int64)
    core, reach = np.asarray(core, np.float32), np.asarray(reach, np.float32)
    iy, ix = np.asarray(iy, np.int64), np.asarray(ix, np.int64)
    thresh = float(thresh)
    S, K = len(first), planes["proposal"].shape[1]
    if cap is None:
        cap = int(tiles.max()) * K
    out = {"count": np.zeros(S, np.int32), "tile": np.zeros((S, cap), np.int32)}
    for name in ("proposal", "cls", "score", "box", "corners"):
        out[name] = np.zeros((S, cap) + planes[name].shape[2:], planes[name].dtype)
    per_class = planes["score"].ndim == 3
    stats = {k: [] for k in ("pairs", "rounds", "kept_guests", "dropped_owned", "most_candidates", "most_above")}
    for s in range(S):
        tile, row, owned = [], [], []
        most = 0
        for t in range(first[s], first[s] + tiles[s]):
            c = int(planes["count"][t])
            xy = np.asarray(planes["box"][t, :c, 0:2], np.float32)
            x, y = xy[:, 0], xy[:, 1]
            cand = (reach[t, 0] <= x) & (x < reach[t, 1]) & (reach[t, 2] <= y) & (y < reach[t, 3])
            own = cand & (core[t, 0] <= x) & (x < core[t, 1]) & (core[t, 2] <= y) & (y < core[t, 3])
            rs = np.nonzero(cand)[0]
            most = max(most, len(rs))
            tile += [t] * len(rs)
            row += rs.tolist()
            owned += own[rs].tolist()
        tile, row, owned = np.array(tile, np.int64), np.array(row, np.int64), np.array(owned, bool)
        cls = planes["cls"][tile, row].astype(np.int64)
        key = np.asarray(planes["score"][tile, row, cls] if per_class else planes["score"][tile, row], np.float32)
        order = np.lexsort((row, tile, -key))  # key descending, then tile, then packed row
        tile, row, owned, cls, key = tile[order], row[order], owned[order], cls[order], key[order]
        corners = np.asarray(planes["corners"][tile, row], np.float32).reshape(-1, 8, 3)
        lo, hi = corners.min(1).astype(np.float64), corners.max(1).astype(np.float64)
        ext = hi - lo
        area = ext[:, 0] * ext[:, 2] if dims == 2 else ext[:, 0] * ext[:, 1] * ext[:, 2]
        n = len(tile)
        winner, partners, above = np.zeros(n, bool), np.zeros(n, np.int64), np.zeros(n, np.int64)
        rounds = np.zeros(n, np.int64)
        for i in range(n):  # row i against every row j above it
            j = slice(0, i)
            d = np.minimum(hi[j], hi[i]) - np.maximum(lo[j], lo[i])
            d = np.where(d > 0, d, 0.0)
            inter = d[:, 0] * d[:, 2] if dims == 2 else d[:, 0] * d[:, 1] * d[:, 2]
            with np.errstate(divide="ignore", invalid="ignore"):
                o = inter / area[i] if old_type else inter / (area[j] + area[i] - inter)
                if same_class:
                    o = o * (cls[j] == cls[i]).astype(np.float64)
                near = (tile[j] != tile[i]) & (np.abs(iy[tile[j]] - iy[tile[i]]) <= 1) & \
                    (np.abs(ix[tile[j]] - ix[tile[i]]) <= 1)
                p = np.nonzero(near & (o > thresh))[0]  # 0 / 0 is NaN: compares false
            partners[i] += len(p)
            partners[p] += 1
            above[i] = len(p)
            winner[i] = not winner[p].any()
            if len(p):
                rounds[i] = (rounds[p].max() if winner[i] else rounds[p[winner[p]]].min()) + 1
        kept = winner & (owned | (partners > 0))
        ks = np.nonzero(kept)[0]
        ks = ks[np.lexsort((row[ks], tile[ks]))]  # tile store order, then packed order
        c = len(ks)
        out["count"][s] = c
        out["tile"][s, :c] = tile[ks]
        for name in ("proposal", "cls", "score", "box", "corners"):
            out[name][s, :c] = planes[name][tile[ks], row[ks]]
        for k, v in (("pairs", int(partners.sum()) // 2), ("rounds", int(rounds.max()) if n else 0),
                     ("kept_guests", int((kept & ~owned).sum())), ("dropped_owned", int((owned & ~kept).sum())),
                     ("most_candidates", most), ("most_above", int(above.max()) if n else 0)):
            stats[k].append(v)
    if info is not None:
        info.update(stats)
    return out


def seam_scratch_bytes(S, T, K, max_tiles):
    """scene_detections_merge_nms_scratch_bytes"""
    from .. import _lib
    return int(_lib.lib.scene_detections_merge_nms_scratch_bytes(S, T, K, max_tiles))


def merge_nms_gpu(merged, tile_arena, first, tiles, core, iy, ix, reach, S, T, K, NC, cap, max_tiles, thresh,
                  old_type, same_class, dims, scratch=None):
    """Launch scene_detections_merge_nms: merge_gpu's arguments plus iy, ix (T,) int32, reach (T, 4)
    float32 on the arenas' device and the four settings (seam_settings); `scratch`: a float64
    tensor of at least seam_scratch_bytes(S, T, K, max_tiles) bytes, allocated here when None
    (uninitialised: the launches write every word they read)."""
    from .. import _lib
    who = "scene_detections_merge_nms"
    if K > MAX_K:
        raise ValueError("%s: K = %d rows per tile, at most %d" % (who, K, MAX_K))
    if cap < max_tiles * K:
        raise ValueError("%s: cap = %d rows per scan, %d tiles of %d need %d" % (who, cap, max_tiles, K, max_tiles * K))
    if dims not in (2, 3) or (dims == 2 and same_class):
        raise ValueError("%s: dims = %r (2 or 3) with same_class = %r (3-D only)" % (who, dims, same_class))
    lin, words_in = arena_layout(T, K, NC)
    lout, words_out = merged_layout(S, cap, NC)
    for name, t, words in (("tile arena", tile_arena, words_in), ("merged arena", merged, words_out)):
        if t.dtype != torch.float32 or t.numel() != words or not t.is_contiguous() or t.device != merged.device:
            raise ValueError("%s: the %s does not match (S, T, K, C, cap) = (%d, %d, %d, %d, %d)"
                             % (who, name, S, T, K, NC, cap))
    for name, t, dtype, shape in (("first", first, torch.int32, (S,)), ("tiles", tiles, torch.int32, (S,)),
                                  ("core", core, torch.float32, (T, 4)), ("iy", iy, torch.int32, (T,)),
                                  ("ix", ix, torch.int32, (T,)), ("reach", reach, torch.float32, (T, 4))):
        if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != merged.device:
            raise ValueError("%s: %s must be %s %s on %s" % (who, name, dtype, shape, merged.device))
    need = seam_scratch_bytes(S, T, K, max_tiles)
    if scratch is None:
        scratch = torch.empty((need + 7) // 8, dtype=torch.float64, device=merged.device)
    if scratch.dtype != torch.float64 or not scratch.is_contiguous() or scratch.device != merged.device or \
            scratch.numel() * 8 < need:
        raise ValueError("%s: the scratch must be float64, contiguous, %d bytes on %s" % (who, need, merged.device))
    a = records.ScanSeamArgs()
    a.S, a.K, a.NC, a.cap, a.max_tiles = S, K, NC, cap, max_tiles
    a.first, a.tiles, a.core = first.data_ptr(), tiles.data_ptr(), core.data_ptr()
    a.iy, a.ix, a.reach = iy.data_ptr(), ix.data_ptr(), reach.data_ptr()
    a.thresh, a.old_type, a.same_class, a.dims = float(thresh), int(old_type), int(same_class), int(dims)
    a.scratch, a.scratch_bytes = scratch.data_ptr(), scratch.numel() * 8
    for plane in PLANES:
        setattr(a, plane + "_in", tile_arena.data_ptr() + 4 * lin[plane][0])
    for plane in MERGED_PLANES:
        setattr(a, plane, merged.data_ptr() + 4 * lout[plane][0])
    _lib.run(who, a, merged.device)
    return merged
