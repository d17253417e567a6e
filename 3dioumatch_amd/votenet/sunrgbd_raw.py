"""Raw SUN RGB-D `sunrgbd_trainval/` folders -> the prepared layout and the store rows, on the GPU.

The reference needs sunrgbd/sunrgbd_data.py --gen_v1_data before any scene can be used: it turns
`depth/%06d.mat` and `label_v1/%06d.txt` into `<id>_pc.npz`, `<id>_bbox.npy` and `<id>_votes.npz` with
scipy, cv2 and mayavi imported, a Python loop over every object and point, and np.random.choice from
global state.  Here the depth clouds are read with zlib and numpy (`read_mat_points`), the label files
become the box table on the host (`read_labels`: at most 64 rows a scene, and np.arctan2 has no
bit-equal device counterpart), and the per-point work of a CHUNK of scenes is three launches
(csrc/sunrgbd_raw.hip, include/sunrgbd_raw_hip.h) between one upload and one copy back
(`export_trainval`): the subsample, the floor height of the kept points, the float32 store rows.
`host_export_trainval_scene` restates the export in numpy: the CPU path and the yardstick of the
device path.  The vote rows are not made here: a store built from this export computes them from the
boxes (sunrgbd_data.SunRgbdScenes, votes="boxes").

Input, as the reference's extract_rgbd_data_v{1,2}.m leave it (calib/ and image/ are not read:
extract_sunrgbd_data reads neither):

  depth/%06d.mat       variable `instance`, (n, 6) xyz + rgb in 0..1, single or double
  label_v1/%06d.txt    (use_v1) or label/%06d.txt: one object a line, 13 space-separated fields
  train_data_idx.txt, val_data_idx.txt   one integer a line

Subsampling: the reference keeps np.random.choice(n, num_point, replace=n < num_point) from global
state (sunrgbd_data.py:226, pc_util.random_sampling).  Here scene number i of the list keeps
scene_loader.sample_indices(seed, 0, i, DRAW_STUDENT, n, num_point) -- distinct for n >= num_point,
with replacement otherwise; the device computes the same function (csrc/scene_common.h) -- or the
explicit `choices[name]`.

The store rows are sunrgbd_data.read_scene's, on the kept rows and in the FILE's dtype: rgb - 0.5,
floor = np.percentile(z, 0.99), height = z - floor, then one rounding to float32.  float32 files
compute the floor in float32 (the arithmetic of scan_data.host_floor), float64 files in float64.

Zero sign: numpy's partition compares -0.0 and +0.0 equal, so where an order statistic is a zero
np.percentile's sign is unspecified.  `host_floor` and the device select on the order-preserving
integer image, where -0.0 comes first: they agree bit for bit, and with np.percentile under ==.

Stricter than the reference, each a SceneError naming the scene: a label line that has not 13 fields
or a non-numeric one, a non-finite label value, more than MAX_NUM_OBJ kept boxes, NaN or Inf in a
cloud.  A scene with no kept box is kept (--gen_v1_data passes skip_empty_scene=False).
"""
import os
import struct
import zlib

import numpy as np
import torch

from .. import records
from .scene_loader import DRAW_STUDENT, MAX_NUM_OBJ, SceneError, explicit_indices, launch, sample_indices, to_device

NUM_POINT = 50000  # sunrgbd_data.py --gen_v1_data / --gen_v2_data
# sunrgbd_utils.py:21 type2class; its keys in this order are sunrgbd_data.py:29 DEFAULT_TYPE_WHITELIST
TYPE2CLASS = {'bed': 0, 'table': 1, 'sofa': 2, 'chair': 3, 'toilet': 4, 'desk': 5, 'dresser': 6, 'night_stand': 7,
              'bookshelf': 8, 'bathtub': 9}
# Raw points per device chunk.  A depth cloud has about 300 000 points, 24 or 48 bytes each, so a chunk
# is about 14 scenes and at most 200 MB on the host and as much again in the packed upload; it also
# keeps every row index of a chunk far inside 32 bits.  A larger scene is a chunk of its own.
CHUNK_POINTS = 1 << 22
KEEP_DRAWN, KEEP_GIVEN = 0, 1  # SUNRAW_KEEP_*
ROW_COLS = 7                   # SUNRAW_ROW_COLS: x y z, r g b - 0.5, z - floor

# ------------------------------------------------------------------ Level-5 MAT files
_MI = {1: "i1", 2: "u1", 3: "<i2", 4: "<u2", 5: "<i4", 6: "<u4", 7: "<f4", 9: "<f8", 12: "<i8", 13: "<u8"}
_MI_OF = {np.dtype(v).str.lstrip("|<"): k for k, v in _MI.items()}
_MI_MATRIX, _MI_COMPRESSED = 14, 15
_MX_SPARSE, _MX_DOUBLE, _MX_SINGLE = 5, 6, 7
_MX_CLASS = {_MX_DOUBLE: np.float64, _MX_SINGLE: np.float32}


def _scan_of(path):
    name = os.path.basename(path)
    return name[:-4] if name.endswith(".mat") else name


def _element(buf, at, what):
    """The data element at buf[at:] -> (type, its data, the offset behind it and its padding)."""
    if at + 8 > len(buf):
        raise SceneError("%s: truncated inside a data element's tag" % what)
    word, size = struct.unpack_from("<II", buf, at)
    if word >> 16:  # the small form: type and size share the first word, the data is the second
        kind, size, start, stop = word & 0xFFFF, word >> 16, at + 4, at + 8
        if size > 4:
            raise SceneError("%s: a small data element of %d bytes" % (what, size))
    else:
        kind, start = word, at + 8
        stop = start + (size if kind == _MI_COMPRESSED else (size + 7) // 8 * 8)
    if start + size > len(buf):
        raise SceneError("%s: truncated: a data element of %d bytes, %d are left" % (what, size, len(buf) - start))
    return kind, buf[start:start + size], min(stop, len(buf))


def _matrix(body, what, wanted):
    """A miMATRIX element's body -> (name, array or None when the name is not `wanted`)."""
    kind, flags, at = _element(body, 0, what)
    if kind != 6 or len(flags) != 8:
        raise SceneError("%s: a matrix without array flags" % what)
    word = struct.unpack_from("<I", flags)[0]
    mx_class, complex_, logical = word & 0xFF, bool(word & 0x0800), bool(word & 0x0200)
    kind, dims, at = _element(body, at, what)
    if kind != 5:
        raise SceneError("%s: a matrix without dimensions" % what)
    dims = np.frombuffer(dims, "<i4")
    kind, name, at = _element(body, at, what)
    if kind != 1:
        raise SceneError("%s: a matrix without a name" % what)
    name = name.decode("latin-1")
    if name != wanted:
        return name, None
    if mx_class == _MX_SPARSE:
        raise SceneError("%s: %r is sparse" % (what, name))
    if mx_class not in _MX_CLASS:
        raise SceneError("%s: %r has class %d, expected double (6) or single (7)" % (what, name, mx_class))
    if complex_ or logical:
        raise SceneError("%s: %r is %s" % (what, name, "complex" if complex_ else "logical"))
    if dims.size != 2 or (dims < 0).any():
        raise SceneError("%s: %r has dimensions %s, expected two" % (what, name, dims.tolist()))
    kind, real, at = _element(body, at, what)
    if kind not in _MI:
        raise SceneError("%s: the real part of %r has storage type %d" % (what, name, kind))
    # the storage type may be narrower than the class: MATLAB stores integral doubles as integers
    stored = np.frombuffer(real, _MI[kind], len(real) // np.dtype(_MI[kind]).itemsize)
    rows, cols = int(dims[0]), int(dims[1])
    if stored.size != rows * cols or len(real) % stored.dtype.itemsize:
        raise SceneError("%s: truncated: %r is %d x %d but holds %d values" % (what, name, rows, cols, stored.size))
    return name, np.ascontiguousarray(stored.astype(_MX_CLASS[mx_class]).reshape(cols, rows).T)  # column-major


def read_mat_points(path, name="instance", columns=(6,)):
    """The real, full, double or single matrix `name` of a Level-5 MAT file (little-endian; top-level
    elements compressed or plain; other variables are skipped) as a C-contiguous (n, columns) array
    in the file's class, float32 or float64.  zlib and numpy only.  Anything else is a SceneError
    naming the scan (the file's name without .mat)."""
    scan = _scan_of(path)
    what = "scan %s: %s" % (scan, path)
    if not os.path.exists(path):
        raise SceneError("scan %s: missing %s" % (scan, path))
    with open(path, "rb") as f:
        buf = f.read()
    if len(buf) < 128:
        raise SceneError("%s: truncated: %d bytes, the header has 128" % (what, len(buf)))
    if buf[126:128] == b"MI":
        raise SceneError("%s: big-endian MAT files are not read" % what)
    if buf[126:128] != b"IM" or not buf.startswith(b"MATLAB 5.0 MAT-file"):
        raise SceneError("%s: not a Level-5 MAT file" % what)
    at, seen = 128, []
    while at < len(buf):
        kind, body, at = _element(buf, at, what)
        if kind == _MI_COMPRESSED:
            try:
                inner = zlib.decompress(body)
            except zlib.error as e:
                raise SceneError("%s: truncated or corrupt compressed element: %s" % (what, e))
            kind, body, _ = _element(inner, 0, what)
        if kind != _MI_MATRIX:
            continue
        found, array = _matrix(body, what, name)
        seen.append(found)
        if array is not None:
            if columns is not None and array.shape[1] not in columns:
                raise SceneError("%s: %r has %d columns, expected %s"
                                 % (what, name, array.shape[1], " or ".join(str(c) for c in columns)))
            return array
    raise SceneError("%s: no variable %r (it holds %s)" % (what, name, ", ".join(repr(s) for s in seen) or "nothing"))


def _tagged(kind, data):
    if 0 < len(data) <= 4:
        return struct.pack("<I", kind | len(data) << 16) + data + b"\0" * (4 - len(data))
    return struct.pack("<II", kind, len(data)) + data + b"\0" * (-len(data) % 8)


def write_mat(path, array, compress=True, name="instance", storage=None):
    """A Level-5 MAT file with the one 2-D float32 or float64 matrix `name`, as MATLAB's save -v7
    (compress) or -v6 writes it.  `storage`: a narrower numpy type for the real part, as MATLAB picks
    for integral values (the values must survive the cast)."""
    array = np.asarray(array)
    if array.ndim != 2 or array.dtype not in (np.float32, np.float64):
        raise ValueError("write_mat: a 2-D float32 or float64 array")
    stored = array.T.reshape(-1)  # column-major
    if storage is not None:
        narrow = stored.astype(storage)
        if not np.array_equal(narrow.astype(array.dtype), stored):
            raise ValueError("write_mat: the values do not survive storage as %s" % np.dtype(storage))
        stored = narrow
    stored = stored.astype(stored.dtype.newbyteorder("<"))
    mx_class = _MX_DOUBLE if array.dtype == np.float64 else _MX_SINGLE
    body = (_tagged(6, struct.pack("<II", mx_class, 0)) + _tagged(5, struct.pack("<ii", *array.shape)) +
            _tagged(1, name.encode("latin-1")) + _tagged(_MI_OF[stored.dtype.str.lstrip("|<")], stored.tobytes()))
    element = struct.pack("<II", _MI_MATRIX, len(body)) + body
    if compress:
        packed = zlib.compress(element)
        element = struct.pack("<II", _MI_COMPRESSED, len(packed)) + packed
    text = b"MATLAB 5.0 MAT-file, written by votenet/sunrgbd_raw.py"
    with open(path, "wb") as f:
        f.write(text + b" " * (124 - len(text)) + struct.pack("<H", 0x0100) + b"IM" + element)


# ------------------------------------------------------------------ label files
def read_labels(path, name=None):
    """The (K, 8) float64 box table of one label file: the kept objects in file order as
    sunrgbd_data.py:209-223 stacks them, [cx, cy, cz, l, w, h, heading, class] with the fields of
    sunrgbd_utils.py:41-59 SUNObject3d (w = field 8, l = field 9, h = field 10, heading =
    -arctan2(field 12, field 11)) and the class of TYPE2CLASS; every other class is dropped."""
    name = name if name is not None else os.path.splitext(os.path.basename(path))[0]
    if not os.path.exists(path):
        raise SceneError("scan %s: missing %s" % (name, path))
    rows = []
    with open(path) as f:
        for number, line in enumerate(f, 1):
            data = line.rstrip().split(' ')
            try:
                if len(data) != 13:
                    raise ValueError("%d fields" % len(data))
                v = [float(x) for x in data[1:]]
            except ValueError as e:
                raise SceneError("scan %s: %s line %d is malformed (%s), expected a class and 12 numbers"
                                 % (name, path, number, e))
            if not np.isfinite(v).all():
                raise SceneError("scan %s: %s line %d holds NaN or Inf" % (name, path, number))
            if data[0] not in TYPE2CLASS:
                continue
            rows.append([v[4], v[5], v[6], v[8], v[7], v[9], -1 * np.arctan2(v[11], v[10]), TYPE2CLASS[data[0]]])
    if len(rows) > MAX_NUM_OBJ:
        raise SceneError("scan %s: %d boxes, at most MAX_NUM_OBJ = %d" % (name, len(rows), MAX_NUM_OBJ))
    return np.array(rows, np.float64).reshape(-1, 8)


# ------------------------------------------------------------------ one scene's files
def scene_name(idx_or_name):
    """'%06d' of a data index (an int, or its decimal text)."""
    try:
        return "%06d" % int(idx_or_name)
    except (TypeError, ValueError):
        raise SceneError("scan %r: a SUN RGB-D scene is named by its integer data index" % (idx_or_name,))


def read_idx_list(path):
    """train_data_idx.txt / val_data_idx.txt -> the scene names."""
    if not os.path.isfile(path):
        raise SceneError("index list %s: no such file" % path)
    with open(path) as f:
        return [scene_name(x.strip()) for x in f.read().splitlines() if x.strip()]


def read_trainval_scene(trainval_dir, idx_or_name, use_v1=True):
    """The raw record of one scene, validated: {"name", "points" (n, 6) float32 or float64 as the depth
    file has them, "boxes" (K, 8) float64}."""
    name = scene_name(idx_or_name)
    points = read_mat_points(os.path.join(trainval_dir, "depth", name + ".mat"))
    n = points.shape[0]
    if n == 0 or n >= 1 << 30:
        raise SceneError("scan %s: %d points" % (name, n))
    boxes = read_labels(os.path.join(trainval_dir, "label_v1" if use_v1 else "label", name + ".txt"), name)
    return {"name": name, "points": points, "boxes": boxes}


# ------------------------------------------------------------------ the choice of kept points
def _choice(rec, num_point, choices):
    """(SUNRAW_KEEP_* mode, explicit indices or None) of one scene."""
    given = None if choices is None else choices.get(rec["name"])
    if given is None:
        return KEEP_DRAWN, None
    return KEEP_GIVEN, explicit_indices(given, np.array([rec["points"].shape[0]]), num_point, rec["name"], "scan's")[0]


# ------------------------------------------------------------------ the numpy restatement
def _order_keys(z):
    """The order-preserving unsigned image of a float array (csrc/scene_common.h order_key)."""
    u = np.ascontiguousarray(z).view(np.uint32 if z.dtype == np.float32 else np.uint64)
    top = u.dtype.type(1) << u.dtype.type(u.dtype.itemsize * 8 - 1)
    return np.where(u & top, ~u, u | top)


def _from_order_keys(k, dtype):
    top = k.dtype.type(1) << k.dtype.type(k.dtype.itemsize * 8 - 1)
    return np.where(k & top, k & ~top, ~k).view(dtype)


def host_floor(z):
    """np.percentile(z, 0.99) restated in z's own dtype, float32 or float64: the two order statistics
    of numpy's linear method and its interpolation (numpy.lib._function_base_impl._quantile / _lerp),
    every operation rounded to the dtype.  The order statistics are taken on the integer image, so
    -0.0 sorts before +0.0: bit-equal to the device, and to np.percentile apart from a zero's sign."""
    z = np.asarray(z).reshape(-1)
    if z.dtype not in (np.float32, np.float64):
        raise ValueError("host_floor: float32 or float64, got %s" % z.dtype)
    n = z.shape[0]
    if n == 0:
        raise ValueError("host_floor: an empty cloud")
    f = z.dtype.type
    q = f(0.99) / f(100)
    v = f(q * f(n - 1))
    lo = min(int(np.floor(v)), n - 1)
    hi = min(lo + 1, n - 1)
    g = f(v - f(lo))
    part = np.partition(_order_keys(z), sorted({lo, hi}))
    a, b = _from_order_keys(part[[lo, hi]], z.dtype)
    with np.errstate(all="ignore"):
        d = f(b - a)
        if g >= f(0.5):
            return f(b - f(d * f(f(1) - g)))
        return f(a + f(d * g))


def store_rows(kept):
    """sunrgbd_data.read_scene's rows of a kept (n, 6) cloud in its own dtype -> (floor, (n, 7)
    float32 = xyz, rgb - 0.5, z - floor)."""
    cloud = np.array(kept[:, 0:6])
    cloud[:, 3:] = cloud[:, 3:] - np.array([0.5, 0.5, 0.5])
    floor = host_floor(cloud[:, 2])
    with np.errstate(all="ignore"):
        height = cloud[:, 2] - floor
    return floor, np.ascontiguousarray(np.concatenate([cloud, height[:, None]], 1), np.float32)


def _refuse_nonfinite(names, nonfinite):
    bad = ["%s (%d)" % (s, c) for s, c in zip(names, nonfinite) if c]
    if bad:
        raise SceneError("scans with NaN or Inf coordinates or colours (count): " + ", ".join(bad))


def host_export_trainval_scene(rec, num_point=NUM_POINT, seed=0, scan_index=0, choice=None):
    """extract_sunrgbd_data (sunrgbd_data.py:200-230) and read_scene's rule for one raw record in
    numpy: {"pc" (num_point, 6) in the file's dtype, "bbox" (K, 8) float64, "floor" a scalar of the
    file's dtype, "rows" (num_point, 7) float32}."""
    points = rec["points"]
    _refuse_nonfinite([rec["name"]], [int((~np.isfinite(points)).sum())])
    n = points.shape[0]
    keep = choice if choice is not None else sample_indices(seed, 0, scan_index, DRAW_STUDENT, n, num_point)
    kept = np.ascontiguousarray(points[keep])
    floor, rows = store_rows(kept)
    return {"pc": kept, "bbox": np.array(rec["boxes"], np.float64).reshape(-1, 8), "floor": floor, "rows": rows}


# ------------------------------------------------------------------ the device export
def _layout(sections):
    """[(name, bytes)] -> ({name: offset}, total), every section on a 16-byte boundary."""
    at, total = {}, 0
    for name, size in sections:
        at[name] = total
        total += (size + 15) // 16 * 16
    return at, max(total, 16)


def _stage_chunk(chunk, device, num_point, seed, choices):
    """One chunk [(scan_index, record)] of ONE dtype on the device, ready to launch: the one upload,
    the block of every output, the filled args record."""
    recs = [r for _, r in chunk]
    S, N = len(recs), int(num_point)
    dtype = recs[0]["points"].dtype
    modes = [_choice(r, N, choices) for r in recs]
    count = np.array([r["points"].shape[0] for r in recs], np.int64)
    raw_offset = np.concatenate([[0], np.cumsum(count, dtype=np.int64)]).astype(np.int64)
    P, Q = int(raw_offset[-1]), S * N
    if P >= 1 << 31 or Q >= 1 << 31:
        raise SceneError("a chunk of %d raw points and %d kept ones" % (P, Q))
    choice = np.zeros(Q, np.int32)
    for s, (mode, given) in enumerate(modes):
        if mode == KEEP_GIVEN:
            choice[s * N:(s + 1) * N] = given
    inputs = [("raw", np.concatenate([r["points"] for r in recs]) if S > 1 else recs[0]["points"]),
              ("raw_offset", raw_offset), ("keep", np.array([m for m, _ in modes], np.int32)),
              ("scan_index", np.array([i for i, _ in chunk], np.int32)), ("choice", choice)]
    at, total = _layout([(k, v.nbytes) for k, v in inputs])
    packed = np.zeros(total, np.uint8)
    for k, v in inputs:
        packed[at[k]:at[k] + v.nbytes] = np.ascontiguousarray(v).reshape(-1).view(np.uint8)
    upload = to_device(packed, device)  # the one upload
    outputs = [("kept", Q * 6 * dtype.itemsize), ("floor", S * dtype.itemsize), ("rows", Q * ROW_COLS * 4),
               ("nonfinite", S * 8)]
    out_at, out_total = _layout(outputs)
    out = torch.empty(out_total // 8, dtype=torch.float64, device=device)  # every output, one block
    a = records.SunRgbdRawArgs()
    a.S, a.num_point, a.elem, a.seed, a.P = S, N, int(dtype == np.float64), int(seed) & 0xFFFFFFFF, P
    for k, _ in inputs:
        setattr(a, k, upload.data_ptr() + at[k])
    for k, _ in outputs:
        setattr(a, k, out.data_ptr() + out_at[k])
    return {"args": a, "device": device, "tensors": [upload, out], "out": out, "out_at": out_at, "recs": recs,
            "sizes": (S, N), "dtype": dtype}


def _launch_staged(staged, fresh=True):
    """scene_sunrgbd_raw_export on the current stream; `fresh`: the chunk's memory was allocated for this call."""
    launch("scene_sunrgbd_raw_export", staged["args"], staged["tensors"] if fresh else [], None, staged["device"])


def _collect(staged):
    """The one copy back of a launched chunk -> the scenes' arrays; a scene with NaN or Inf is refused here."""
    (S, N), out_at, recs, dtype = staged["sizes"], staged["out_at"], staged["recs"], staged["dtype"]
    host = staged["out"].cpu().numpy().view(np.uint8)

    def part(k, dt, size):
        return host[out_at[k]:out_at[k] + size * np.dtype(dt).itemsize].view(dt)

    kept, rows = part("kept", dtype, S * N * 6).reshape(S, N, 6), part("rows", np.float32, S * N * ROW_COLS).reshape(S, N, ROW_COLS)
    floor, nonfinite = part("floor", dtype, S), part("nonfinite", np.uint64, S)
    _refuse_nonfinite([r["name"] for r in recs], nonfinite)
    return [{"pc": np.array(kept[s]), "bbox": np.array(r["boxes"], np.float64).reshape(-1, 8), "floor": floor[s],
             "rows": np.array(rows[s])} for s, r in enumerate(recs)]


def _export_chunk(chunk, device, num_point, seed, choices):
    staged = _stage_chunk(chunk, device, num_point, seed, choices)
    _launch_staged(staged)
    return _collect(staged)


def export_trainval(records, device, num_point=NUM_POINT, seed=0, choices=None, first_index=0,
                    chunk_points=CHUNK_POINTS):
    """`records` (an iterable of read_trainval_scene's records; a generator keeps one chunk of raw
    clouds in host memory at a time) -> a list of {"pc" (num_point, 6) in the file's dtype, "bbox"
    (K, 8) float64, "floor", "rows" (num_point, 7) float32}.  Per chunk -- consecutive scenes of one
    dtype, at most `chunk_points` raw points -- one upload, the launches of scene_sunrgbd_raw_export,
    one copy back.  `device=None`: host_export_trainval_scene.  A scene keeps `choices[name]`
    (num_point indices, checked here) or the draw (seed, 0, first_index + its place in `records`,
    DRAW_STUDENT)."""
    num_point = int(num_point)
    if num_point < 1:
        raise ValueError("num_point >= 1")
    out, chunk, points = [], [], 0
    for index, rec in enumerate(records, int(first_index)):
        if rec["boxes"].shape[0] > MAX_NUM_OBJ:
            raise SceneError("scan %s: %d boxes, at most MAX_NUM_OBJ = %d" % (rec["name"], rec["boxes"].shape[0], MAX_NUM_OBJ))
        if rec["points"].dtype not in (np.float32, np.float64) or rec["points"].ndim != 2 or rec["points"].shape[1] != 6:
            raise SceneError("scan %s: the cloud is %s %s, expected (n, 6) float32 or float64"
                             % (rec["name"], rec["points"].dtype, rec["points"].shape))
        n = rec["points"].shape[0]
        if n == 0 or n >= 1 << 30:
            raise SceneError("scan %s: %d points" % (rec["name"], n))
        if device is None:
            out.append(host_export_trainval_scene(rec, num_point, seed, index, _choice(rec, num_point, choices)[1]))
            continue
        if chunk and (points + n > chunk_points or chunk[0][1]["points"].dtype != rec["points"].dtype):
            out += _export_chunk(chunk, torch.device(device), num_point, seed, choices)
            chunk, points = [], 0
        chunk.append((index, rec))
        points += n
    if chunk:
        out += _export_chunk(chunk, torch.device(device), num_point, seed, choices)
    return out


def save_export(out_dir, name, arrays):
    """`<name>_pc.npz` ('pc', the file's dtype) and `<name>_bbox.npy` as sunrgbd_data.py:228-230 writes them."""
    np.savez_compressed(os.path.join(out_dir, name + "_pc.npz"), pc=arrays["pc"])
    np.save(os.path.join(out_dir, name + "_bbox.npy"), arrays["bbox"])


# ------------------------------------------------------------------ synthetic trainval folders
def write_label_file(path, objects):
    """`objects`: [(classname, (cx, cy, cz), (l, w, h), heading)] -> one 13-field line each (the 2-D
    box is zeros; repr keeps every float64 exactly)."""
    with open(path, "w") as f:
        for classname, centre, (l, w, h), heading in objects:
            v = [0.0, 0.0, 0.0, 0.0] + [float(c) for c in centre] + [float(w), float(l), float(h),
                                                                     float(np.cos(-heading)), float(np.sin(-heading))]
            f.write(" ".join([classname] + [repr(x) for x in v]) + "\n")


def synthetic_trainval(folder, count, points=300000, boxes=12, seed=0, dtype=np.float32):
    """A seeded stand-in `sunrgbd_trainval/` (for tools/ and tests, where no dataset is at hand): scenes
    1..count with depth/, label_v1/ and label/ (the same objects; one in five of a class outside the
    whitelist), the last quarter in val_data_idx.txt and the rest in train_data_idx.txt.  Two thirds of
    the points fall inside a box.  -> the scene names."""
    g = np.random.default_rng(seed)
    for sub in ("depth", "label_v1", "label"):
        os.makedirs(os.path.join(folder, sub), exist_ok=True)
    kinds = sorted(TYPE2CLASS)
    names = [scene_name(i) for i in range(1, count + 1)]
    for name in names:
        box = np.zeros((boxes, 7))
        box[:, 0:3] = g.random((boxes, 3)) * [5.0, 4.0, 1.5] + [-2.5, 1.0, -1.0]
        box[:, 3:6] = g.random((boxes, 3)) * 0.6 + 0.15
        box[:, 6] = g.random(boxes) * 2 * np.pi - np.pi
        xyz = g.random((points, 3)) * [6.0, 5.0, 2.5] + [-3.0, 0.5, -1.3]
        if boxes:
            inside = np.where(g.random(points) < 2.0 / 3.0)[0]
            b = g.integers(0, boxes, inside.size)
            local = (g.random((inside.size, 3)) * 2 - 1) * box[b, 3:6]
            c, s = np.cos(box[b, 6]), np.sin(box[b, 6])
            xyz[inside, 0] = box[b, 0] + local[:, 0] * c + local[:, 1] * s
            xyz[inside, 1] = box[b, 1] - local[:, 0] * s + local[:, 1] * c
            xyz[inside, 2] = box[b, 2] + local[:, 2]
        cloud = np.concatenate([xyz, g.random((points, 3))], 1).astype(dtype)
        write_mat(os.path.join(folder, "depth", name + ".mat"), cloud)
        objects = [(kinds[int(g.integers(0, len(kinds)))] if k % 5 != 4 else "lamp", r[0:3], r[3:6], r[6])
                   for k, r in enumerate(box)]
        for sub in ("label_v1", "label"):
            write_label_file(os.path.join(folder, sub, name + ".txt"), objects)
    n_val = max(1, count // 4) if count > 1 else 0
    for split, part in (("train", names[:count - n_val]), ("val", names[count - n_val:])):
        with open(os.path.join(folder, split + "_data_idx.txt"), "w") as f:
            f.write("".join("%d\n" % int(s) for s in part))
    return names
