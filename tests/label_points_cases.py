"""Cases the CPU and the GPU tests of label_points share (test_label_points.py,
test_label_points_gpu.py): hand-made arenas in both layouts (Detections: cap = K; TiledDetections:
cap = max_tiles * K with the `tile` plane) and the clouds they label.  Every array comes from a fixed
seed; a 6-column cloud is its 3-column one with colours behind it.  The host results (`want`) are
computed once per case, columns and prefer mode and shared: do not write to them.

  sizes      scans of 1, B - 1, B, B + 1 and 3 B + 1 points (B = LABEL_BLOCK) in one store -- a one-point
             scan next to a three-block one -- with 0, 1, 3, cap and 5 rows.
  chunks     the tiled layout with per-class scores: scans with CH - 1, CH, CH + 1 and cap rows
             (CH = LABEL_BOX_CHUNK).
  ownership  nested boxes, identical boxes with equal keys, a row under a min_score, and a row
             ineligible by each of: NaN key, negative key, zero size, Inf size, NaN heading.
  faces      points on the faces and corners of a heading-0 box with representable half sizes, and one
             float32 step outside; the same for boxes turned by 0.3 and -2.5.
  cull       a box far from every point, a box whose bounding sphere just touches the workgroup's
             bounding box at a point on its corner, a box around the whole cloud; the cloud in sorted
             and in shuffled order.
  geometric  random oriented boxes and clouds with every point within 1e-4 m of a face plane removed:
             the labels equal a float64 evaluation exactly.
"""
import importlib

import numpy as np

from conftest import load_pkg

load_pkg()
D = importlib.import_module("3dioumatch_amd.votenet.detect")
PL = importlib.import_module("3dioumatch_amd.votenet.point_labels")

F = np.float32
B, CH = PL.LABEL_BLOCK, PL.LABEL_BOX_CHUNK
PREFERS = ("score", "smallest")
SIZES = (1, B - 1, B, B + 1, 3 * B + 1)
SIZES_ROWS = (0, 1, 3, 8, 5)  # cap = K = 8
CHUNK_K, CHUNK_TILES = 129, 2  # cap = 258 >= CH + 1
CHUNK_ROWS = (CH - 1, CH, CH + 1, CHUNK_K * CHUNK_TILES)
GEOMETRIC_SEEDS = (71, 72)
FACE_MARGIN = 1e-4


class Parents(object):
    """What TiledDetections reads of its store"""

    def __init__(self, names):
        self.parent_names = list(names)


def _with_colour(xyz, columns, seed):
    xyz = np.ascontiguousarray(xyz, F)
    if columns == 3:
        return xyz
    rgb = np.random.default_rng(seed).integers(0, 256, (len(xyz), 3)).astype(F)
    return np.ascontiguousarray(np.concatenate([xyz, rgb], 1))


def _room(g, n):
    return (g.random((n, 3)) * [4.0, 4.0, 2.0] - [2.0, 2.0, 0.0]).astype(F)


def _random_boxes(g, n, lo=0.3, hi=2.5):
    """(n, 7) float32 oriented boxes over _room's extent"""
    centre = g.random((n, 3)) * [4.0, 4.0, 2.0] - [2.0, 2.0, 0.0]
    size = lo + g.random((n, 3)) * (hi - lo)
    heading = g.random((n, 1)) * 2 * np.pi - np.pi
    return np.concatenate([centre, size, heading], 1).astype(F)


def _planes(S, cap, NC):
    return {"count": np.zeros(S, np.int32), "cls": np.zeros((S, cap), np.int32),
            "score": np.zeros((S, cap, NC) if NC else (S, cap), F), "box": np.zeros((S, cap, 7), F)}


def _fill_random(planes, s, rows, g, NC):
    planes["count"][s] = rows
    planes["box"][s, :rows] = _random_boxes(g, rows)
    planes["cls"][s, :rows] = g.integers(0, NC + 1 if NC else 18, rows)  # with NC: one class in NC + 1 is out of range
    planes["score"][s, :rows] = g.random(planes["score"][s, :rows].shape).astype(F)


# ------------------------------------------------------------------ the cases
def sizes_case():
    g = np.random.default_rng(51)
    planes = _planes(len(SIZES), 8, 0)
    for s, rows in enumerate(SIZES_ROWS):
        _fill_random(planes, s, rows, g, 0)
    clouds = [_room(g, n) for n in SIZES]
    clouds[0][0] = planes["box"][1, 0, 0:3]  # (the one-point scan has no rows; scan 1's one row holds its centre)
    clouds[1][7] = planes["box"][1, 0, 0:3]
    return {"layout": "plain", "K": 8, "cap": 8, "NC": 0, "planes": planes, "clouds": clouds}


def chunks_case():
    g = np.random.default_rng(52)
    NC, cap = 3, CHUNK_K * CHUNK_TILES
    planes = _planes(len(CHUNK_ROWS), cap, NC)
    for s, rows in enumerate(CHUNK_ROWS):
        _fill_random(planes, s, rows, g, NC)
        planes["box"][s, :rows, 3:6] *= F(0.35)  # many small boxes: most rows own something
    planes["tile"] = np.zeros((len(CHUNK_ROWS), cap), np.int32)
    for s, rows in enumerate(CHUNK_ROWS):
        planes["tile"][s, :rows] = np.sort(g.integers(0, CHUNK_TILES, rows))
    clouds = [_room(g, n) for n in (B + 44, 2 * B, 300, B + 1)]
    for s, rows in enumerate(CHUNK_ROWS):  # the LAST row of every scan: the best key and the smallest box, on point 0
        planes["box"][s, rows - 1] = list(clouds[s][0]) + [0.05, 0.05, 0.05, 0.4]
        planes["score"][s, rows - 1], planes["cls"][s, rows - 1] = 2.0, 0
    return {"layout": "tiled", "K": CHUNK_K, "cap": cap, "NC": NC, "planes": planes, "clouds": clouds}


# rows of ownership_case by name
OWN = {"table": 0, "mug": 1, "twin_a": 2, "twin_b": 3, "faint": 4, "nan_key": 5, "negative_key": 6, "zero_size": 7,
       "inf_size": 8, "nan_heading": 9, "floor": 10}
OWN_ROWS = 11
OWN_MIN_SCORE = 0.3  # above `faint` (0.2) and `floor` (0.1)
# the centre of the region each ineligible row would own (all inside `floor`)
OWN_SPOTS = {"nan_key": (6.0, 0.0), "negative_key": (6.0, 1.0), "zero_size": (6.0, 2.0), "inf_size": (6.0, 3.0),
             "nan_heading": (6.0, 4.0)}


def ownership_case():
    """One scan.  `mug` (score 0.5, small) sits inside `table` (score 0.9, large): score -> table,
    smallest -> mug.  twin_a and twin_b are bit-identical with equal keys: the lower row.  `faint`
    (score 0.2) owns its points until min_score rises above it.  The five ineligible rows each sit on
    a spot inside `floor` (score 0.1, the largest box) and would outrank it -- a NaN or negative key
    has larger bits than 0.1, a zero or infinite size the smallest or an unordered volume -- so their
    points go to `floor`, or to nothing once min_score is above it.  Rows 11..15 are past count."""
    g = np.random.default_rng(53)
    planes = _planes(1, 16, 0)
    box, score = planes["box"][0], planes["score"][0]
    box[OWN["table"]] = [0.0, 0.0, 0.5, 2.0, 1.0, 1.0, 0.3]
    box[OWN["mug"]] = [0.2, 0.1, 0.8, 0.2, 0.2, 0.2, -1.0]
    box[OWN["twin_a"]] = box[OWN["twin_b"]] = [3.0, 0.0, 0.5, 1.0, 1.0, 1.0, 0.7]
    box[OWN["faint"]] = [0.0, 3.0, 0.5, 1.0, 1.0, 1.0, 0.0]
    for name, (x, y) in OWN_SPOTS.items():
        box[OWN[name]] = [x, y, 0.5, 0.5, 0.5, 0.5, 0.1]
    box[OWN["zero_size"], 3] = 0.0
    box[OWN["inf_size"], 4] = np.inf
    box[OWN["nan_heading"], 6] = np.nan
    box[OWN["floor"]] = [6.0, 2.0, 0.5, 2.0, 6.0, 1.0, 0.0]
    score[:OWN_ROWS] = [0.9, 0.5, 0.6, 0.6, 0.2, np.nan, -0.95, 0.8, 0.8, 0.8, 0.1]
    planes["cls"][0, :OWN_ROWS] = [4, 7, 2, 3, 5, 1, 1, 1, 1, 1, 9]
    planes["count"][0] = OWN_ROWS
    parts = [box[OWN["table"], 0:3] + (g.random((300, 3)) - 0.5) * [2.4, 1.6, 1.2],
             box[OWN["mug"], 0:3] + (g.random((60, 3)) - 0.5) * 0.3,
             box[OWN["twin_a"], 0:3] + (g.random((80, 3)) - 0.5) * 1.4,
             box[OWN["faint"], 0:3] + (g.random((80, 3)) - 0.5) * 1.2]
    for x, y in OWN_SPOTS.values():
        parts.append(np.array([[x, y, 0.5]]))  # the centre itself: inside a box of size 0 along x
        parts.append(np.array([x, y, 0.5]) + (g.random((30, 3)) - 0.5) * 0.6)
    return {"layout": "plain", "K": 16, "cap": 16, "NC": 0, "planes": planes,
            "clouds": [np.concatenate(parts).astype(F)]}


FACE_BOX = (2.0, 4.0, 1.0, 1.0, 0.5, 0.25)  # centre, size: half sizes 0.5, 0.25, 0.125; no face coordinate is finer than its half size
FACE_ON = 14       # the first rows of the faces cloud lie ON the heading-0 box: inside
FACE_OUTSIDE = 14  # the next rows are those one float32 step outward along one axis: outside


def _on_box(centre, half):
    """the 6 face centres and 8 corners of an upright box"""
    pts = []
    for a in range(3):
        for sign in (-1.0, 1.0):
            p = np.array(centre, np.float64)
            p[a] += sign * half[a]
            pts.append(p)
    for sx in (-1.0, 1.0):
        for sy in (-1.0, 1.0):
            for sz in (-1.0, 1.0):
                pts.append(np.array(centre, np.float64) + np.array([sx, sy, sz]) * half)
    return np.array(pts)


def faces_case():
    """Row 0: the heading-0 box; rows 1, 2: boxes turned by 0.3 and -2.5 elsewhere.  The cloud: the
    14 points on row 0 (exact in float32), each stepped outward along one axis, then for each turned box
    its 14 surface points rounded to float32, stepped both ways along x, and points scattered about."""
    g = np.random.default_rng(54)
    planes = _planes(1, 4, 0)
    centre, size = np.array(FACE_BOX[0:3]), np.array(FACE_BOX[3:6])
    planes["box"][0, 0] = list(FACE_BOX) + [0.0]
    planes["box"][0, 1] = [5.0, 2.0, 0.5, 1.0, 0.5, 0.25, 0.3]
    planes["box"][0, 2] = [9.0, 2.0, 0.5, 1.0, 0.5, 0.25, -2.5]
    planes["score"][0, :3] = [0.5, 0.6, 0.7]
    planes["cls"][0, :3] = [1, 2, 3]
    planes["count"][0] = 3
    on = _on_box(centre, size / 2).astype(F)
    assert np.array_equal(on.astype(np.float64), _on_box(centre, size / 2))  # representable
    out = on.copy()
    for i, p in enumerate(_on_box(np.zeros(3), size / 2)):
        a = int(np.argmax(np.abs(p) > 0))  # the first axis along which the point is off-centre
        out[i, a] = np.nextafter(on[i, a], F(np.inf * np.sign(p[a])))
    parts = [on, out]
    for row in (1, 2):
        b = planes["box"][0, row].astype(np.float64)
        local = _on_box(np.zeros(3), b[3:6] / 2)
        c, s = np.cos(b[6]), np.sin(b[6])  # x' = c dx - s dy, z' = s dx + c dy: dx = c x' + s z', dy = c z' - s x'
        world = np.stack([c * local[:, 0] + s * local[:, 1], c * local[:, 1] - s * local[:, 0], local[:, 2]], 1) + b[0:3]
        w = world.astype(F)
        up, down = w.copy(), w.copy()
        up[:, 0], down[:, 0] = np.nextafter(w[:, 0], F(np.inf)), np.nextafter(w[:, 0], F(-np.inf))
        parts += [w, up, down, (b[0:3] + (g.random((60, 3)) - 0.5) * [1.6, 1.2, 0.4]).astype(F)]
    return {"layout": "plain", "K": 4, "cap": 4, "NC": 0, "planes": planes, "clouds": [np.concatenate(parts).astype(F)]}


CULL = {"far": 0, "touch": 1, "around": 2, "touch_turned": 3}
CULL_SIDE = 16  # 16 x 16 x 4 = 1024 grid points: four workgroups in sorted order


def cull_case():
    """Two scans of the same 1024 points of [0, 1]^3 (a grid, so (1, 1, 1) is one of them): in x-major
    sorted order, where workgroup 3 holds the slab x >= 0.8, and shuffled.  `touch` is an upright box
    whose corner is (1, 1, 1): its bounding sphere touches every workgroup box that holds that point at
    exactly its radius, and the point is inside (a corner).  `touch_turned` does the same turned by 0.3
    at the corner (0, 0, 0) as well as float32 lets it.  `far` is 1000 m away, `around` contains
    everything; some small boxes inside make the owners vary."""
    g = np.random.default_rng(55)
    n = CULL_SIDE
    ax, az = np.linspace(0.0, 1.0, n), np.linspace(0.0, 1.0, 4)
    grid = np.stack(np.meshgrid(ax, ax, az, indexing="ij"), -1).reshape(-1, 3).astype(F)
    assert len(grid) == 4 * B and (grid[-1] == 1).all() and (grid[0] == 0).all()
    planes = _planes(2, 16, 0)
    box = planes["box"][0]
    box[CULL["far"]] = [1000.0, -1000.0, 0.5, 1.0, 1.0, 1.0, 0.4]
    box[CULL["touch"]] = [1.5, 1.25, 1.125, 1.0, 0.5, 0.25, 0.0]
    box[CULL["around"]] = [0.5, 0.5, 0.5, 3.0, 3.0, 3.0, 1.0]
    c, s = np.cos(0.3), np.sin(0.3)  # the corner (+hl, +hw, +hh) of the turned box sits on the origin
    box[CULL["touch_turned"]] = [-(c * 0.5 + s * 0.25), -(c * 0.25 - s * 0.5), -0.125, 1.0, 0.5, 0.25, 0.3]
    box[4:12] = _random_boxes(g, 8, 0.1, 0.5)
    box[4:12, 0:3] = g.random((8, 3))
    planes["score"][0, :12] = [0.9, 0.8, 0.1, 0.85] + list(0.2 + 0.05 * np.arange(8))
    planes["cls"][0, :12] = np.arange(12)
    planes["count"][0] = 12
    for k in planes:
        planes[k][1] = planes[k][0]
    return {"layout": "plain", "K": 16, "cap": 16, "NC": 0, "planes": planes,
            "clouds": [grid, grid[cull_permutation()]]}


def cull_permutation():
    return np.random.default_rng(56).permutation(4 * B)


def float64_margin(xyz, box):
    """(n, rows) float64: max(|x'| - hl, |z'| - hw, |dz| - hh) of every point against every box, all
    in float64 from the float32 values -- negative inside -- and the least distance to a face plane."""
    p, b = np.asarray(xyz, np.float64)[:, None, 0:3], np.asarray(box, np.float64)[None]
    c, s = np.cos(b[..., 6]), np.sin(b[..., 6])
    d = p - b[..., 0:3]
    q = np.stack([np.abs(c * d[..., 0] - s * d[..., 1]), np.abs(s * d[..., 0] + c * d[..., 1]), np.abs(d[..., 2])], -1)
    off = q - b[..., 3:6] / 2
    return off.max(-1), np.abs(off).min(-1)


def geometric_case(seed):
    """Two scans, 24 and 40 random oriented boxes, about 1500 points each after the points within
    FACE_MARGIN of any face plane of any box of their scan are removed.  `generated` keeps the counts
    before the removal."""
    g = np.random.default_rng(seed)
    rows = (24, 40)
    planes = _planes(2, 40, 0)
    clouds, generated = [], []
    for s, r in enumerate(rows):
        _fill_random(planes, s, r, g, 0)
        planes["box"][s, :r, 3:6] *= F(0.6)
        xyz = _room(g, 1500 + 200 * s)
        _, face = float64_margin(xyz, planes["box"][s, :r])
        generated.append(len(xyz))
        clouds.append(np.ascontiguousarray(xyz[(face >= FACE_MARGIN).all(1)]))
    return {"layout": "plain", "K": 40, "cap": 40, "NC": 0, "planes": planes, "clouds": clouds, "generated": generated}


def float64_labels(case, prefer):
    """The owners by a pure float64 evaluation: membership by float64_margin <= 0, the rank of the
    rule (keys and volumes are float32 values of the planes).  Only for cases whose rows are all
    eligible.  -> flat (P,) int32"""
    c = get(case)
    out = []
    for s, cloud in enumerate(c["clouds"]):
        r = int(c["planes"]["count"][s])
        box = c["planes"]["box"][s, :r]
        inside = float64_margin(cloud, box)[0] <= 0
        if prefer == "score":
            order = np.lexsort((np.arange(r), -c["planes"]["score"][s, :r].astype(np.float64)))
        else:
            order = np.lexsort((np.arange(r), ((box[:, 3] * box[:, 4]) * box[:, 5]).astype(np.float64)))
        owner = np.full(len(cloud), -1, np.int32)
        for row in order[::-1]:  # the best row is written last
            owner[inside[:, row]] = row
        out.append(owner)
    return np.concatenate(out)


CASES = {"sizes": sizes_case, "chunks": chunks_case, "ownership": ownership_case, "faces": faces_case,
         "cull": cull_case}
CASES.update({"geometric%d" % seed: (lambda seed=seed: geometric_case(seed)) for seed in GEOMETRIC_SEEDS})
MIN_SCORES = {"ownership": (0.0, OWN_MIN_SCORE)}  # the min_score values a case is run at (default: 0 only)

_cases, _want = {}, {}


def get(case):
    """The case (shared: do not write to it)."""
    if case not in _cases:
        c = CASES[case]()
        for a in list(c["planes"].values()) + c["clouds"]:
            a.setflags(write=False)
        c["names"] = ["%s_%d" % (case, s) for s in range(len(c["clouds"]))]
        _cases[case] = c
    return _cases[case]


def clouds(case, columns=3):
    return [_with_colour(x, columns, 60 + i) for i, x in enumerate(get(case)["clouds"])]


def min_scores(case):
    return MIN_SCORES.get(case, (0.0,))


GARBAGE = ("nan", "huge")


def planes(case, garbage=None):
    """The case's planes; with `garbage` the rows past count hold NaN or huge finite values in place
    of zeros (a fresh copy)."""
    c = get(case)
    if garbage is None:
        return c["planes"]
    out = {k: v.copy() for k, v in c["planes"].items()}
    past = np.arange(c["cap"])[None, :] >= out["count"][:, None]
    out["box"][past] = np.nan if garbage == "nan" else F(3e38)
    out["score"][past] = np.nan if garbage == "nan" else F(3e38)
    out["cls"][past] = -1 if garbage == "nan" else (1 << 30)
    return out


def arena(case, garbage=None):
    """The flat float32 arena of the case in its layout (proposal and corners zero)."""
    c, p = get(case), planes(case, garbage)
    S = len(c["clouds"])
    layout, words = D.arena_layout(S, c["K"], c["NC"]) if c["layout"] == "plain" else D.merged_layout(S, c["cap"], c["NC"])
    flat = np.zeros(words, F)
    for name, (at, shape) in layout.items():
        if name in p:
            a = np.ascontiguousarray(p[name])
            assert a.shape == tuple(shape), (name, a.shape, shape)
            flat[at:at + a.size] = (a.view(F) if a.dtype == np.int32 else a).reshape(-1)
    return flat


def found(case, arena_array, num_class=18):
    """A Detections or TiledDetections over `arena_array` (numpy, or a device tensor of arena(case))."""
    c = get(case)
    if c["layout"] == "plain":
        return D.Detections(arena_array, c["names"], c["K"], c["NC"], num_class)
    return D.TiledDetections(arena_array, Parents(c["names"]), c["cap"], c["K"], c["NC"], num_class)


def want(case, prefer, min_score=0.0):
    """host_label_points of the case, computed once."""
    key = (case, prefer, float(min_score))
    if key not in _want:
        got = PL.host_label_points(planes(case), get(case)["clouds"], prefer, min_score)
        for a in got.values():
            a.setflags(write=False)
        _want[key] = got
    return _want[key]
