"""Raw ScanNet scan folders -> the four arrays of the preprocessed layout, labels and boxes on the GPU.

The reference needs scannet/batch_load_scannet_data.py before any scan can be used: it turns
`<scan>_vh_clean_2.ply`, `<scan>.aggregation.json`, `<scan>_vh_clean_2.0.010000.segs.json` and
`<scan>.txt` into `<scan>_vert.npy`, `_ins_label.npy`, `_sem_label.npy` and `_bbox.npy`, with the
`plyfile` package and Python loops over every vertex and segment.  Here the files are read with numpy
and the standard library (`read_ply_vertices`, `read_raw_scan`), the two JSON files are reduced to
tables over segment ids (`seg_tables`), and the per-vertex and per-object work of a CHUNK of scans is
four launches (csrc/scannet_raw.hip, include/scannet_raw_hip.h) between one upload and one copy back
(`export_raw_scans`).  `host_export_raw_scan` restates the export in numpy from the reference's text:
the CPU path and the yardstick of the device path.

The seg tables (line numbers: scannet/load_scannet_data.py).  With `segGroups` in file order, group g
= (objectId + 1, label, segments):

  seg_label[s]     int32, length max seg id + 1, 0 = unannotated: the nyu40 id of the LAST label
                   group that lists segment s, where label groups are ordered by the first
                   appearance of their label in segGroups (the insertion order of label_to_segs,
                   :38-41, walked at :88-92) and, within a label, keep file order (:39 extends).
  seg_object[s]    int32, 0 = none: objectId + 1 of the LAST group in file order that lists s
                   (object_id_to_segs is walked in insertion order, :95-98).
  object_label[o]  seg_label[first segment of object o's group] (:99-100): every vertex of a segment
                   carries that segment's final label, so `label_ids[verts][0]` is a table lookup.

A vertex's instance id is seg_object[segIndices[v]], its semantic id seg_label[segIndices[v]].

Stricter than the reference, each a SceneError naming the scan: a group without segments (the
reference raises KeyError at :103 unless an aliased list was extended), two groups with one objectId
(the reference keeps the dictionary position of the first and the segments of the last), non-finite
coordinates or matrix entries (the integer images the extents are reduced on order finite floats).

Subsampling: the reference draws np.random.choice(N, MAX_NUM_POINT, replace=False) from global state
(batch_load_scannet_data.py:69-74).  Here a scan with more than `max_points` vertices keeps
scene_loader.sample_indices(seed, 0, scan_index, DRAW_STUDENT, n, max_points) -- distinct indices, the
device computes the same function (csrc/scene_common.h) -- or the explicit `choices[name]`.
"""
import csv
import json
import os

import numpy as np
import torch

from .. import records
from .scene_loader import (DRAW_STUDENT, MAX_NUM_OBJ, SceneError, explicit_indices, launch, sample_indices,
                           to_device)

MAX_INSTANCES = 1024   # objects per scan (SNR_MAX_OBJECTS, scannet_data.MAX_INSTANCES)
MAX_NUM_POINT = 50000  # batch_load_scannet_data.py:36
OBJ_CLASS_IDS = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39])  # :35
# batch_load_scannet_data.py:34,57-60 masks the vertices whose semantic id is in this list.  It is
# empty in the reference, so the mask keeps every vertex; neither path has a branch for it.
DONOTCARE_CLASS_IDS = np.array([])
# Vertices per device chunk.  ScanNet v2 meshes average about 150 000 vertices, so a chunk is about
# 26 scans: 28 bytes a vertex raw, 112 MB on the host and as much again in the packed upload, where
# the train split's 1201 scans would be about 5 GB at once.  It also keeps every row index of a
# chunk far inside 32 bits.  A larger scan is a chunk of its own.
CHUNK_POINTS = 1 << 22
KEEP_ALL, KEEP_DRAWN, KEEP_GIVEN = 0, 1, 2  # SNR_KEEP_*

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2",
              "ushort": "u2", "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4",
              "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}
SUFFIXES = {"mesh": "_vh_clean_2.ply", "agg": ".aggregation.json", "seg": "_vh_clean_2.0.010000.segs.json",
            "meta": ".txt"}


# ------------------------------------------------------------------ the mesh file
def _ply_header(f, path):
    """-> (format, [[element, count, [(property, numpy type)], has a list property]])"""
    if f.readline().strip() != b"ply":
        raise SceneError("%s: not a PLY file" % path)
    fmt, elements = None, []
    while True:
        line = f.readline()
        if not line:
            raise SceneError("%s: the header is truncated (no end_header)" % path)
        words = line.decode("ascii", "replace").split()
        if not words or words[0] in ("comment", "obj_info"):
            continue
        if words[0] == "end_header":
            break
        try:
            if words[0] == "format":
                fmt = words[1]
            elif words[0] == "element":
                elements.append([words[1], int(words[2]), [], False])
            elif words[0] == "property":
                if words[1] == "list":
                    elements[-1][3] = True
                else:
                    elements[-1][2].append((words[2], _PLY_TYPES[words[1]]))
            else:
                raise SceneError("%s: unknown header line %r" % (path, " ".join(words)))
        except (IndexError, KeyError, ValueError):
            raise SceneError("%s: malformed header line %r" % (path, " ".join(words)))
    return fmt, elements


def read_ply_vertices(path):
    """The `vertex` element of a PLY file (binary_little_endian 1.0 or ascii 1.0) as (n, 3) float32
    x y z or, when the file has red green blue, (n, 6) with the colours as stored (0..255 for
    ScanNet's uchar).  Other properties (alpha, normals) are ignored and nothing behind the vertices
    (the faces) is read."""
    if not os.path.exists(path):
        raise SceneError("%s: no such file" % path)
    with open(path, "rb") as f:
        fmt, elements = _ply_header(f, path)
        if fmt == "binary_big_endian":
            raise SceneError("%s: big-endian PLY files are not read" % path)
        if fmt not in ("binary_little_endian", "ascii"):
            raise SceneError("%s: format %r, expected binary_little_endian or ascii" % (path, fmt))
        binary = fmt == "binary_little_endian"
        vertex = None
        for name, count, props, has_list in elements:
            if name == "vertex":
                vertex = (count, props, has_list)
                break
            if not binary:
                for _ in range(count):
                    f.readline()
            elif has_list:
                raise SceneError("%s: the element %r with a list property comes before the vertices" % (path, name))
            else:
                f.seek(count * sum(np.dtype(t).itemsize for _, t in props), 1)
        if vertex is None:
            raise SceneError("%s: no vertex element" % path)
        count, props, has_list = vertex
        names = [p for p, _ in props]
        if has_list or len(set(names)) != len(names):
            raise SceneError("%s: the vertex element has a list property or a repeated property" % path)
        for c in "xyz":
            if c not in names:
                raise SceneError("%s: the vertices have no property %r" % (path, c))
        if binary:
            dtype = np.dtype([(p, "<" + t) for p, t in props])
            data = f.read(count * dtype.itemsize)
            if len(data) < count * dtype.itemsize:
                raise SceneError("%s: truncated: %d vertices declared, %d bytes of %d"
                                 % (path, count, len(data), count * dtype.itemsize))
            table = np.frombuffer(data, dtype, count)
            column = lambda p: table[p]  # noqa: E731
        else:
            lines = [f.readline() for _ in range(count)]
            if count and not lines[-1].strip():
                raise SceneError("%s: truncated: %d vertices declared" % (path, count))
            try:
                values = np.array(b" ".join(lines).split(), np.float64)
            except ValueError:
                raise SceneError("%s: a vertex line is not numeric" % path)
            if values.size != count * len(names):
                raise SceneError("%s: truncated: %d values for %d vertices of %d properties"
                                 % (path, values.size, count, len(names)))
            values = values.reshape(count, len(names))
            column = lambda p: values[:, names.index(p)]  # noqa: E731
        cols = ["x", "y", "z"] + (["red", "green", "blue"] if all(c in names for c in ("red", "green", "blue")) else [])
        out = np.zeros((count, len(cols)), np.float32)
        for k, p in enumerate(cols):
            out[:, k] = column(p)
        return out


# ------------------------------------------------------------------ labels
def read_label_map(tsv, label_from="raw_category", label_to="nyu40id"):
    """scannet_utils.read_label_mapping (scannet/scannet_utils.py:34-43): a column of the labels tsv ->
    another, as int; integer-looking keys become ints as there."""
    if not os.path.isfile(tsv):
        raise SceneError("label map %s: no such file" % tsv)
    mapping = {}
    with open(tsv, newline="") as f:
        for row in csv.DictReader(f, delimiter="\t"):
            if label_from not in row or label_to not in row:
                raise SceneError("label map %s: no column %r or %r" % (tsv, label_from, label_to))
            mapping[row[label_from]] = int(row[label_to])
    if mapping:
        try:
            int(next(iter(mapping)))
            mapping = {int(k): v for k, v in mapping.items()}
        except ValueError:
            pass
    return mapping


def _last_wins(table, index, value):
    """table[index] = value where a repeated index keeps its LAST value (numpy does not promise an
    order for repeated indices in one assignment)."""
    if index.size:
        u, first = np.unique(index[::-1], return_index=True)
        table[u] = value[::-1][first]


def seg_tables(name, seg, groups, label_map):
    """(seg_label, seg_object, object_label) of one scan (see the module docstring) from its
    segIndices and its groups [(objectId, label, segments)] in file order, after validating every
    index a kernel will follow; a failure is a SceneError naming the scan."""
    seg = np.asarray(seg)
    if seg.ndim != 1 or seg.size == 0 or seg.dtype.kind not in "iu":
        raise SceneError("scan %s: segIndices is not a list of integers" % name)
    if int(seg.min()) < 0:
        raise SceneError("scan %s: a negative segment id %d" % (name, int(seg.min())))
    if int(seg.max()) >= 1 << 30:
        raise SceneError("scan %s: segment id %d" % (name, int(seg.max())))
    length = int(seg.max()) + 1
    present = np.bincount(seg, minlength=length) > 0
    oid = np.array([g[0] for g in groups], np.int64) + 1
    objects = np.unique(oid).size
    if objects > MAX_INSTANCES:
        raise SceneError("scan %s: %d objects, at most MAX_INSTANCES = %d" % (name, objects, MAX_INSTANCES))
    if objects != oid.size:
        raise SceneError("scan %s: two segGroups share an objectId" % name)
    if oid.size and (int(oid.min()) < 1 or int(oid.max()) > objects):
        bad = oid[(oid < 1) | (oid > objects)][0]
        raise SceneError("scan %s: objectId + 1 = %d outside 1..%d, the number of distinct object ids"
                         % (name, bad, objects))
    segs, ids, rank = [], np.zeros(len(groups), np.int32), np.zeros(len(groups), np.int64)
    first_seen = {}
    for g, (_, label, members) in enumerate(groups):
        s = np.asarray(members)
        if s.ndim != 1 or s.size == 0 or s.dtype.kind not in "iu":
            raise SceneError("scan %s: the group of object %d has no list of segments" % (name, oid[g] - 1))
        s = s.astype(np.int64)
        if (s < 0).any() or (s >= length).any() or not present[s].all():
            bad = [int(x) for x in s if x < 0 or x >= length or not present[x]][0]
            raise SceneError("scan %s: object %d lists segment %d, which no vertex carries" % (name, oid[g] - 1, bad))
        if label not in label_map:
            raise SceneError("scan %s: the label %r of object %d is not in the label map" % (name, label, oid[g] - 1))
        if not 0 <= int(label_map[label]) < 1 << 31:
            raise SceneError("scan %s: the label %r maps to %r" % (name, label, label_map[label]))
        segs.append(s)
        ids[g] = int(label_map[label])
        rank[g] = first_seen.setdefault(label, len(first_seen))
    seg_label, seg_object = np.zeros(length, np.int32), np.zeros(length, np.int32)
    object_label = np.zeros(objects, np.int32)
    if segs:
        counts = np.array([s.size for s in segs])
        # :39-41 make label_to_segs[label] the very list of the label's first object, which later
        # objects of that label extend, so that object is walked over their segments too (:95-98).
        # It changes nothing: each later object comes after it in file order and overwrites them.
        _last_wins(seg_object, np.concatenate(segs), np.repeat(oid.astype(np.int32), counts))
        order = np.argsort(rank, kind="stable")
        _last_wins(seg_label, np.concatenate([segs[g] for g in order]), np.repeat(ids[order], counts[order]))
        object_label[oid - 1] = seg_label[np.array([s[0] for s in segs])]
    return seg_label, seg_object, object_label


# ------------------------------------------------------------------ one scan's files
def _scan_paths(scan_dir, name):
    folder = os.path.join(scan_dir, name)
    if not os.path.isdir(folder):
        folder = scan_dir  # the scan's own folder was given
    paths = {k: os.path.join(folder, name + suffix) for k, suffix in SUFFIXES.items()}
    for p in paths.values():
        if not os.path.exists(p):
            raise SceneError("scan %s: missing %s" % (name, p))
    return paths


def _load_json(name, path, key):
    try:
        with open(path) as f:
            data = json.load(f)
        return data[key]
    except (ValueError, KeyError, TypeError) as e:
        raise SceneError("scan %s: %s: %s" % (name, path, e))


def read_raw_scan(scan_dir, name, label_map):
    """The raw record of the scan `name` under `scan_dir` (`scan_dir/name/name_vh_clean_2.ply` ..., or
    `scan_dir` the scan's own folder), validated: {"name", "vert" (n, 6) float32 xyz and rgb 0..255,
    "seg" (n,) int32 segIndices, "groups" [(objectId, label, segments)] in file order, "matrix" (4, 4)
    float64 axisAlignment, "seg_label", "seg_object", "object_label" (seg_tables)}.  `label_map`: the
    dict of read_label_map, or the tsv's path."""
    if not isinstance(label_map, dict):
        label_map = read_label_map(label_map)
    paths = _scan_paths(scan_dir, name)
    try:
        vert = read_ply_vertices(paths["mesh"])
    except SceneError as e:
        raise SceneError("scan %s: %s" % (name, e))
    if vert.shape[1] != 6:
        raise SceneError("scan %s: %s has no red green blue" % (name, paths["mesh"]))
    n = vert.shape[0]
    if n == 0 or n >= 1 << 30:
        raise SceneError("scan %s: %d vertices" % (name, n))
    if not np.isfinite(vert[:, 0:3]).all():
        raise SceneError("scan %s: NaN or Inf coordinates" % name)
    matrix = None
    with open(paths["meta"]) as f:
        for line in f:
            if "axisAlignment" in line:  # load_scannet_data.py:71-77
                try:
                    matrix = np.array([float(x) for x in line.split("=", 1)[1].split()], np.float64)
                except (IndexError, ValueError):
                    matrix = np.zeros(0)
                break
    if matrix is None:
        raise SceneError("scan %s: %s has no axisAlignment line" % (name, paths["meta"]))
    if matrix.size != 16 or not np.isfinite(matrix).all():
        raise SceneError("scan %s: axisAlignment is not 16 finite numbers" % name)
    try:
        seg = np.asarray(_load_json(name, paths["seg"], "segIndices"))
        groups = [(int(g["objectId"]), g["label"], g["segments"])
                  for g in _load_json(name, paths["agg"], "segGroups")]
    except (KeyError, TypeError, ValueError) as e:
        raise SceneError("scan %s: malformed segGroups: %r" % (name, e))
    if seg.ndim != 1 or seg.shape[0] != n:
        raise SceneError("scan %s: %d vertices but %d segIndices" % (name, n, seg.shape[0] if seg.ndim else 0))
    seg_label, seg_object, object_label = seg_tables(name, seg, groups, label_map)
    return {"name": name, "vert": vert, "seg": seg.astype(np.int32), "groups": groups,
            "matrix": matrix.reshape(4, 4), "seg_label": seg_label, "seg_object": seg_object,
            "object_label": object_label}


def raw_scan_names(scan_dir):
    """The scans of a raw folder: its sub-folders that hold their mesh file, sorted."""
    return sorted(d for d in os.listdir(scan_dir)
                  if os.path.exists(os.path.join(scan_dir, d, d + SUFFIXES["mesh"])))


# ------------------------------------------------------------------ the choice of kept vertices
def _choice(rec, max_points, choices):
    """(SNR_KEEP_* mode, explicit indices or None) of one scan."""
    n = rec["vert"].shape[0]
    given = None if choices is None else choices.get(rec["name"])
    if n <= max_points:
        if given is not None:
            raise ValueError("scan %s: %d vertices <= max_points = %d, nothing is drawn" % (rec["name"], n, max_points))
        return KEEP_ALL, None
    if given is None:
        return KEEP_DRAWN, None
    return KEEP_GIVEN, explicit_indices(given, np.array([n]), max_points, rec["name"], "scan's")[0]


# ------------------------------------------------------------------ the numpy restatement
def host_export_raw_scan(rec, max_points=MAX_NUM_POINT, seed=0, scan_index=0, choice=None):
    """export (load_scannet_data.py:60-129) and export_one_scan (batch_load_scannet_data.py:49-79) of
    one raw record in numpy: {"vert" (n, 6) float32, "ins_label", "sem_label" uint32, "bbox" (nb, 7)
    float64}.  The float64 sum of the alignment is taken left to right, one rounded operation each,
    where the reference leaves the order to its BLAS."""
    vert = np.array(rec["vert"], np.float32)
    m = np.asarray(rec["matrix"], np.float64)
    x, y, z = (vert[:, k].astype(np.float64) for k in range(3))
    for r in range(3):  # pts = np.dot(pts, axis_align_matrix.transpose()) with pts[:, 3] = 1 (:78-81)
        vert[:, r] = ((x * m[r, 0] + y * m[r, 1]) + z * m[r, 2]) + 1.0 * m[r, 3]
    seg = rec["seg"]
    sem = rec["seg_label"][seg].astype(np.uint32)     # :86-92
    ins = rec["seg_object"][seg].astype(np.uint32)    # :93-98
    objects = rec["object_label"].shape[0]
    bbox = np.zeros((objects, 7))                     # :101
    order = np.argsort(ins, kind="stable")
    ids = np.arange(1, objects + 1)
    start, stop = np.searchsorted(ins[order], ids, "left"), np.searchsorted(ins[order], ids, "right")
    has = stop > start                                # :105
    if has.any():
        xyz = vert[order, 0:3]  # the objects' runs end at the array's end: id 0 sorts in front
        lo, hi = np.minimum.reduceat(xyz, start[has], axis=0), np.maximum.reduceat(xyz, start[has], axis=0)
        bbox[has, 0:3] = (lo + hi) / np.float32(2)    # float32 scalars in the reference (:111-118)
        bbox[has, 3:6] = hi - lo
        bbox[has, 6] = rec["object_label"][has]
    bbox = bbox[np.isin(bbox[:, -1], OBJ_CLASS_IDS)]  # batch_load_scannet_data.py:65-66
    if bbox.shape[0] > MAX_NUM_OBJ:
        raise SceneError("scan %s: %d boxes, at most MAX_NUM_OBJ = %d" % (rec["name"], bbox.shape[0], MAX_NUM_OBJ))
    n = vert.shape[0]
    if n > max_points:                                # :69-74
        keep = choice if choice is not None else sample_indices(seed, 0, scan_index, DRAW_STUDENT, n, max_points)
        vert, ins, sem = vert[keep], ins[keep], sem[keep]
    return {"vert": vert, "ins_label": ins, "sem_label": sem, "bbox": bbox}


# ------------------------------------------------------------------ the device export
def _offsets(counts):
    return np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]).astype(np.int64)


def _layout(sections):
    """[(name, bytes)] -> ({name: offset}, total), every section on a 16-byte boundary."""
    at, total = {}, 0
    for name, size in sections:
        at[name] = total
        total += (size + 15) // 16 * 16
    return at, max(total, 16)


def _stage_chunk(chunk, device, max_points, seed, choices):
    """One chunk [(scan_index, record)] on the device, ready to launch: the one upload, the block of
    every output, the filled args record."""
    recs = [r for _, r in chunk]
    S = len(recs)
    modes = [_choice(r, max_points, choices) for r in recs]
    count = np.array([r["vert"].shape[0] for r in recs], np.int64)
    kept = np.array([c if mode == KEEP_ALL else max_points for c, (mode, _) in zip(count, modes)], np.int64)
    objects = np.array([r["object_label"].shape[0] for r in recs], np.int64)
    vert_offset, out_offset, obj_offset = _offsets(count), _offsets(kept), _offsets(objects)
    seg_offset = _offsets([r["seg_label"].shape[0] for r in recs])
    P, Q, T = int(vert_offset[-1]), int(out_offset[-1]), int(obj_offset[-1])
    if P >= 1 << 31:
        raise SceneError("a chunk of %d vertices" % P)
    choice = np.zeros(Q, np.int32)
    for s, (mode, given) in enumerate(modes):
        if mode == KEEP_GIVEN:
            choice[out_offset[s]:out_offset[s + 1]] = given
    inputs = [("raw", np.concatenate([r["vert"] for r in recs]).astype(np.float32, copy=False)),
              ("seg", np.concatenate([r["seg"] for r in recs]).astype(np.int32, copy=False)),
              ("matrix", np.stack([np.asarray(r["matrix"], np.float64).reshape(16) for r in recs])),
              ("vert_offset", vert_offset), ("seg_offset", seg_offset),
              ("seg_label", np.concatenate([r["seg_label"] for r in recs]).astype(np.int32, copy=False)),
              ("seg_object", np.concatenate([r["seg_object"] for r in recs]).astype(np.int32, copy=False)),
              ("obj_offset", obj_offset),
              ("object_label", np.concatenate([r["object_label"] for r in recs] + [np.zeros(1, np.int32)]).astype(np.int32)),
              ("out_offset", out_offset), ("keep", np.array([m for m, _ in modes], np.int32)),
              ("scan_index", np.array([i for i, _ in chunk], np.int32)), ("choice", choice)]
    at, total = _layout([(k, v.nbytes) for k, v in inputs])
    packed = np.zeros(total, np.uint8)
    for k, v in inputs:
        packed[at[k]:at[k] + v.nbytes] = np.ascontiguousarray(v).reshape(-1).view(np.uint8)
    upload = to_device(packed, device)  # the one upload
    outputs = [("bbox", (T + 1) * 7 * 8), ("vert", Q * 6 * 4), ("ins_label", Q * 4), ("sem_label", Q * 4), ("nbox", S * 4)]
    out_at, out_total = _layout(outputs)
    out = torch.empty(out_total // 8, dtype=torch.float64, device=device)  # every output, one block
    extent = torch.empty((T + 1) * 6, dtype=torch.int32, device=device)
    a = records.ScanNetRawArgs()
    a.S, a.P, a.Q, a.T = S, P, Q, T
    a.max_objects, a.max_points, a.seed = int(objects.max()), int(max_points), int(seed) & 0xFFFFFFFF
    for k, _ in inputs:
        setattr(a, k, upload.data_ptr() + at[k])
    for k, _ in outputs:
        setattr(a, k, out.data_ptr() + out_at[k])
    a.extent = extent.data_ptr()
    return {"args": a, "device": device, "tensors": [upload, out, extent], "out": out, "out_at": out_at,
            "recs": recs, "sizes": (S, Q, T), "out_offset": out_offset, "obj_offset": obj_offset}


def _launch_staged(staged, fresh=True):
    """scannet_raw_export on the current stream; `fresh`: the chunk's memory was allocated for this call."""
    launch("scannet_raw_export", staged["args"], staged["tensors"] if fresh else [], None, staged["device"])


def _collect(staged):
    """The one copy back of a launched chunk -> the scans' arrays."""
    (S, Q, T), out_at, recs = staged["sizes"], staged["out_at"], staged["recs"]
    out_offset, obj_offset = staged["out_offset"], staged["obj_offset"]
    host = staged["out"].cpu().numpy().view(np.uint8)

    def part(k, dtype, size):
        return host[out_at[k]:out_at[k] + size * np.dtype(dtype).itemsize].view(dtype)

    vert, bbox = part("vert", np.float32, Q * 6).reshape(Q, 6), part("bbox", np.float64, (T + 1) * 7).reshape(T + 1, 7)
    ins, sem, nbox = part("ins_label", np.uint32, Q), part("sem_label", np.uint32, Q), part("nbox", np.int32, S)
    results = []
    for s, r in enumerate(recs):
        if nbox[s] > MAX_NUM_OBJ:
            raise SceneError("scan %s: %d boxes, at most MAX_NUM_OBJ = %d" % (r["name"], nbox[s], MAX_NUM_OBJ))
        rows = slice(int(out_offset[s]), int(out_offset[s + 1]))
        results.append({"vert": np.array(vert[rows]), "ins_label": np.array(ins[rows]), "sem_label": np.array(sem[rows]),
                        "bbox": np.array(bbox[obj_offset[s]:obj_offset[s] + nbox[s]]).reshape(-1, 7)})
    return results


def _export_chunk(chunk, device, max_points, seed, choices):
    staged = _stage_chunk(chunk, device, max_points, seed, choices)
    _launch_staged(staged)
    return _collect(staged)


def export_raw_scans(records, device, max_points=MAX_NUM_POINT, seed=0, choices=None, chunk_points=CHUNK_POINTS,
                     first_index=0):
    """`records` (an iterable of read_raw_scan's records; a generator keeps one chunk of raw scans in
    host memory at a time) -> a list of {"vert" (n, 6) float32, "ins_label", "sem_label" (n,) uint32,
    "bbox" (nb, 7) float64}, what batch_load_scannet_data.export_one_scan saves.  Per chunk of at most
    `chunk_points` vertices: one upload, the launches of scannet_raw_export, one copy back.
    `device=None`: host_export_raw_scan.  A scan with more than `max_points` vertices keeps
    `choices[name]` (max_points indices, checked here) or the draw (seed, 0, first_index + its place in
    `records`, DRAW_STUDENT)."""
    max_points = int(max_points)
    if max_points < 1:
        raise ValueError("max_points >= 1")
    out, chunk, points = [], [], 0
    for index, rec in enumerate(records, int(first_index)):
        if device is None:
            out.append(host_export_raw_scan(rec, max_points, seed, index, _choice(rec, max_points, choices)[1]))
            continue
        n = rec["vert"].shape[0]
        if chunk and points + n > chunk_points:
            out += _export_chunk(chunk, torch.device(device), max_points, seed, choices)
            chunk, points = [], 0
        chunk.append((index, rec))
        points += n
    if chunk:
        out += _export_chunk(chunk, torch.device(device), max_points, seed, choices)
    return out


EXPORT_KEYS = ("vert", "ins_label", "sem_label", "bbox")


def save_export(out_dir, name, arrays):
    """The four files of one scan as batch_load_scannet_data.py:76-79 names them."""
    for k in EXPORT_KEYS:
        np.save(os.path.join(out_dir, "%s_%s.npy" % (name, k)), arrays[k])


# ------------------------------------------------------------------ synthetic raw scans
SYNTHETIC_LABELS = {"cabinet": 3, "bed": 4, "chair": 5, "sofa": 6, "table": 7, "door": 8, "wall": 1, "floor": 2}


def synthetic_raw_scan(num_vertices=150000, objects=40, seed=0):
    """A seeded ScanNet-sized stand-in (for tools/ and tests, where no dataset is at hand): (vert (n, 6),
    segIndices, groups, matrix).  Segments are runs of about 100 consecutive vertices, as a mesh's vertex
    order keeps a segment together, with one vertex in fifty elsewhere; each object takes a run of
    segments, one in eight of which stays unannotated; labels are SYNTHETIC_LABELS' keys."""
    g = np.random.default_rng(seed)
    n = int(num_vertices)
    segments = max(objects, n // 100)
    seg = (np.arange(n, dtype=np.int64) * segments // n).astype(np.int32)
    stray = g.random(n) < 0.02
    seg[stray] = g.integers(0, segments, int(stray.sum()))
    seg[np.arange(segments) * n // segments] = np.arange(segments)  # every segment keeps a vertex
    centre = g.random((segments, 3)) * [8.0, 6.0, 2.5]
    xyz = centre[seg] + g.normal(size=(n, 3)) * 0.15
    vert = np.concatenate([xyz, g.integers(0, 256, (n, 3))], 1).astype(np.float32)
    labels = sorted(SYNTHETIC_LABELS)
    per = segments // objects
    groups = [(o, labels[int(g.integers(0, len(labels)))], [s for s in range(o * per, (o + 1) * per) if s % 8 != 7 or per == 1])
              for o in range(objects)]
    t = g.random() * 2 * np.pi
    matrix = np.array([[np.cos(t), -np.sin(t), 0, -4.0], [np.sin(t), np.cos(t), 0, -3.0], [0, 0, 1, -0.05], [0, 0, 0, 1]])
    return vert, seg, groups, matrix


def write_ply(path, vert, binary=True, alpha=True, faces=0):
    """A ScanNet-style mesh file: float x y z, uchar red green blue [alpha], `faces` triangles."""
    vert = np.asarray(vert)
    n, colour = vert.shape[0], vert.shape[1] >= 6
    props = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if colour:
        props += [(c, "u1") for c in ("red", "green", "blue")] + ([("alpha", "u1")] if alpha else [])
    head = ["ply", "format %s 1.0" % ("binary_little_endian" if binary else "ascii"), "comment synthetic",
            "element vertex %d" % n]
    head += ["property %s %s" % ("float" if t == "<f4" else "uchar", p) for p, t in props]
    head += ["element face %d" % faces, "property list uchar int vertex_indices", "end_header"]
    table = np.zeros(n, np.dtype(props))
    for k, (p, _) in enumerate(props):
        table[p] = 255 if p == "alpha" else vert[:, k]
    tri = np.arange(faces * 3, dtype="<i4").reshape(faces, 3) % max(n, 1)
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        if binary:
            f.write(table.tobytes())
            face = np.zeros(faces, np.dtype([("k", "u1"), ("v", "<i4", 3)]))
            face["k"], face["v"] = 3, tri
            f.write(face.tobytes())
        else:
            for row in table:
                f.write((" ".join(repr(float(v)) if isinstance(v, np.floating) else str(int(v)) for v in row) + "\n").encode())
            for t in tri:
                f.write(("3 %d %d %d\n" % tuple(t)).encode())


def write_raw_scan(scan_dir, name, vert, seg, groups, matrix, binary=True):
    """One scan in the raw layout under scan_dir/name/; `groups`: [(objectId, label, segments)]."""
    folder = os.path.join(scan_dir, name)
    os.makedirs(folder, exist_ok=True)
    write_ply(os.path.join(folder, name + SUFFIXES["mesh"]), vert, binary=binary, faces=2)
    with open(os.path.join(folder, name + SUFFIXES["seg"]), "w") as f:
        json.dump({"sceneId": name, "segIndices": [int(s) for s in seg]}, f)
    with open(os.path.join(folder, name + SUFFIXES["agg"]), "w") as f:
        json.dump({"sceneId": name, "segGroups": [{"id": k, "objectId": int(o), "segments": [int(s) for s in m],
                                                   "label": l} for k, (o, l, m) in enumerate(groups)]}, f)
    with open(os.path.join(folder, name + SUFFIXES["meta"]), "w") as f:
        f.write("axisAlignment = %s \n" % " ".join("%f" % v for v in np.asarray(matrix).reshape(-1)))
        f.write("numDepthFrames = 0\n")
