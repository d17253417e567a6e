"""CPU tests of label_points: host_label_points against a point-by-point loop, ownership as a
partition, the prefer modes, the tie rule and the eligibility table on the hand-made arena, the face
points, the cull adversaries in sorted and shuffled order, the geometric builder, what the shared
cases cover, the refusals, the host path of label_points (both layouts, save) and tools/detect.py's
new flags."""
import importlib
import importlib.util
import os

import numpy as np
import pytest

import label_points_cases as cases
from conftest import ROOT, load_pkg
from label_points_cases import B, CH, CULL, OWN, PREFERS

load_pkg()
SC = importlib.import_module("3dioumatch_amd.votenet.scan_data")
D = importlib.import_module("3dioumatch_amd.votenet.detect")
PL = importlib.import_module("3dioumatch_amd.votenet.point_labels")
V = importlib.import_module("3dioumatch_amd.votenet")


def brute_force(planes, cloud, s, prefer, min_score):
    """The rule point by point and row by row with numpy float32 scalars: (owner (n,), points (cap,))."""
    F = np.float32
    cap = planes["cls"].shape[1]
    count = min(max(int(planes["count"][s]), 0), cap)
    rows = []
    for r in range(count):
        cx, cy, cz, l, w, h, heading = (F(v) for v in planes["box"][s, r])
        c, sn = F(np.cos(np.float64(heading))), F(np.sin(np.float64(heading)))
        hl, hw, hh = (F(np.float64(v) / 2) for v in (l, w, h))
        cls = int(planes["cls"][s, r])
        if planes["score"].ndim == 3:
            if not 0 <= cls < planes["score"].shape[2]:
                continue
            key = F(planes["score"][s, r, cls])
        else:
            key = F(planes["score"][s, r])
        if not np.isfinite([c, sn, cx, cy, cz, hl, hw, hh]).all() or not (l > 0 and w > 0 and h > 0):
            continue
        if np.isnan(key) or not np.float64(key) >= max(min_score, 0.0):
            continue
        with np.errstate(over="ignore"):
            high = int(np.abs(key).view(np.uint32)) if prefer == "score" else 0xFFFFFFFF - int(F(F(l * w) * h).view(np.uint32))
        rows.append(((high << 32) | (0xFFFFFFFF - r), r, (c, sn, cx, cy, cz, hl, hw, hh)))
    owner = np.full(len(cloud), -1, np.int32)
    for i, p in enumerate(np.asarray(cloud, F)):
        best = 0
        for rank, r, (c, sn, cx, cy, cz, hl, hw, hh) in rows:
            dx, dy, dz = F(p[0] - cx), F(p[1] - cy), F(p[2] - cz)
            xr = F(F(c * dx) - F(sn * dy))
            zr = F(F(sn * dx) + F(c * dy))
            if abs(xr) <= hl and abs(zr) <= hw and abs(dz) <= hh and rank > best:
                best, owner[i] = rank, r
    return owner, np.bincount(owner[owner >= 0], minlength=cap).astype(np.int32)


def per_scan(case, flat):
    n = [len(c) for c in cases.get(case)["clouds"]]
    return np.split(np.asarray(flat), np.cumsum(n)[:-1])


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("prefer", PREFERS)
@pytest.mark.parametrize("case", ["sizes", "ownership", "faces", "cull", "geometric71"])
def test_host_label_points_is_the_loop(case, prefer):
    c = cases.get(case)
    for min_score in cases.min_scores(case):
        got = cases.want(case, prefer, min_score)
        assert got["instance"].dtype == got["semantic"].dtype == got["points"].dtype == np.int32
        for s, (cloud, inst, sem) in enumerate(zip(c["clouds"], per_scan(case, got["instance"]),
                                                   per_scan(case, got["semantic"]))):
            if len(cloud) > 2 * B:
                cloud, inst, sem = cloud[::5], inst[::5], sem[::5]  # the loop is slow: a fifth of the large scans
                owner, _ = brute_force(c["planes"], cloud, s, prefer, min_score)
            else:
                owner, points = brute_force(c["planes"], cloud, s, prefer, min_score)
                assert np.array_equal(got["points"][s], points), (s, min_score)
            assert np.array_equal(inst, owner), (s, min_score)
            assert np.array_equal(sem, np.where(owner >= 0, c["planes"]["cls"][s][np.maximum(owner, 0)], -1))


@pytest.mark.parametrize("prefer", PREFERS)
@pytest.mark.parametrize("case", sorted(cases.CASES))
def test_ownership_is_a_partition(case, prefer):
    """every point has one owner or none; a row's points are the points labelled with it; the owner
    contains the point and is eligible; no row past count owns anything"""
    c = cases.get(case)
    for min_score in cases.min_scores(case):
        got = cases.want(case, prefer, min_score)
        f = PL.host_frames(c["planes"], prefer, min_score)
        for s, (cloud, inst) in enumerate(zip(c["clouds"], per_scan(case, got["instance"]))):
            count = int(c["planes"]["count"][s])
            assert inst.min() >= -1 and inst.max() < max(count, 0) or (count == 0 and (inst == -1).all())
            assert np.array_equal(got["points"][s], np.bincount(inst[inst >= 0], minlength=c["cap"]))
            assert got["points"][s].sum() + (inst == -1).sum() == len(cloud)
            assert not got["points"][s, count:].any()
            for r in np.unique(inst[inst >= 0]):
                assert f["rank"][s, r] != 0
                assert PL.host_inside(cloud[inst == r], f["frames"][s, r]).all()
            eligible = np.nonzero(f["rank"][s])[0]
            if len(eligible):  # a point with no owner lies in no eligible row
                free = cloud[inst == -1]
                assert not any(PL.host_inside(free, f["frames"][s, r]).any() for r in eligible)


def test_prefer_modes_ties_and_eligibility_on_the_hand_made_arena():
    c = cases.get("ownership")
    cloud, planes = c["clouds"][0], c["planes"]
    f = PL.host_frames(planes, "score", 0.0)
    inside = {name: PL.host_inside(cloud, f["frames"][0, r]) for name, r in OWN.items()}
    by = {p: cases.want("ownership", p)["instance"] for p in PREFERS}
    nested = inside["mug"] & inside["table"]
    assert nested.sum() >= 20 and inside["mug"].sum() == nested.sum()
    assert (by["score"][nested] == OWN["table"]).all() and (by["smallest"][nested] == OWN["mug"]).all()  # they disagree
    assert (by["score"][inside["table"]] == OWN["table"]).all()
    twins = inside["twin_a"]
    assert twins.sum() >= 20 and np.array_equal(twins, inside["twin_b"])
    for p in PREFERS:  # equal keys, identical boxes: the lowest row
        assert (by[p][twins] == OWN["twin_a"]).all() and not (by[p] == OWN["twin_b"]).any()
        assert cases.want("ownership", p)["points"][0, OWN["twin_b"]] == 0
    # the eligibility table
    for p in PREFERS:
        rank = PL.host_frames(planes, p, 0.0)["rank"][0]
        bad = [OWN[k] for k in ("nan_key", "negative_key", "zero_size", "inf_size", "nan_heading")]
        assert not rank[bad].any() and not rank[cases.OWN_ROWS:].any()
        good = [r for r in range(cases.OWN_ROWS) if r not in bad]
        assert rank[good].all() and len(set(rank[good].tolist())) == len(good)
        assert ((rank[good] & np.uint64(0xFFFFFFFF)) == np.uint64(0xFFFFFFFF) - np.array(good, np.uint64)).all()
        for name, (x, y) in cases.OWN_SPOTS.items():  # their points go to `floor`, the only eligible row there
            spot = (np.abs(cloud[:, 0] - x) < 0.31) & (np.abs(cloud[:, 1] - y) < 0.31)
            assert spot.sum() == 31 and (by[p][spot] == OWN["floor"]).all(), name
        centre = np.nonzero((cloud == np.float32([6.0, 2.0, 0.5])).all(1))[0]
        assert len(centre) == 1 and PL.host_inside(cloud[centre], f["frames"][0, OWN["zero_size"]]).all()
        # min_score above `faint` and `floor`: their points are free, everything else stands
        raised = cases.want("ownership", p, cases.OWN_MIN_SCORE)["instance"]
        low = np.isin(by[p], [OWN["faint"], OWN["floor"]])
        assert (by[p] == OWN["faint"]).sum() >= 20 and (raised[low] == -1).all()
        assert np.array_equal(raised[~low], by[p][~low])
        sem = cases.want("ownership", p)["semantic"]
        assert np.array_equal(sem, np.where(by[p] >= 0, planes["cls"][0][np.maximum(by[p], 0)], -1))
    # a negative min_score is 0: a key of -0.95 stays out
    assert np.array_equal(PL.host_label_points(planes, c["clouds"], "score", -5.0)["instance"], by["score"])
    high = PL.host_frames(planes, "score", 0.0)["rank"][0] >> np.uint64(32)
    assert high[OWN["table"]] == np.float32(0.9).view(np.uint32)
    small = PL.host_frames(planes, "smallest", 0.0)["rank"][0] >> np.uint64(32)
    assert small[OWN["mug"]] == 0xFFFFFFFF - int(np.float32(np.float32(np.float32(0.2) * np.float32(0.2)) * np.float32(0.2)).view(np.uint32))


def test_per_class_scores_key_is_the_score_of_the_rows_class():
    c = cases.get("chunks")
    planes = c["planes"]
    assert planes["score"].ndim == 3 and "tile" in planes
    f = PL.host_frames(planes, "score", 0.0)
    S, cap = planes["cls"].shape
    for s in range(S):
        for r in range(0, int(planes["count"][s]), 37):
            cls = int(planes["cls"][s, r])
            if cls < c["NC"]:
                assert f["rank"][s, r] >> np.uint64(32) == planes["score"][s, r, cls].view(np.uint32)
            else:  # a class the scores do not have: ineligible
                assert f["rank"][s, r] == 0
    assert (planes["cls"] >= c["NC"]).any() and (f["rank"] != 0).sum() > 100
    got = cases.want("chunks", "score")
    assert (got["points"] > 0).sum() > 50  # many owners


def test_faces_are_inclusive_and_one_step_outside_is_outside():
    c = cases.get("faces")
    cloud = c["clouds"][0]
    for p in PREFERS:
        inst = cases.want("faces", p)["instance"]
        assert (inst[:cases.FACE_ON] == 0).all()
        assert (inst[cases.FACE_ON:cases.FACE_ON + cases.FACE_OUTSIDE] == -1).all()
        assert (inst == 1).sum() > 20 and (inst == 2).sum() > 20
    f = PL.host_frames(c["planes"], "score", 0.0)["frames"][0]
    assert f[0].tolist() == [1.0, 0.0, 2.0, 4.0, 1.0, 0.5, 0.25, 0.125]
    assert np.allclose(f[1, 0:2], [np.cos(0.3), np.sin(0.3)], atol=1e-7)
    # the stepped copies of the turned boxes' surface points fall on both sides
    near = slice(2 * cases.FACE_ON, 2 * cases.FACE_ON + 3 * 14)
    inst = cases.want("faces", "score")["instance"]
    assert set(inst[near].tolist()) == {-1, 1} and len(cloud) > 200


def test_cull_adversaries_and_the_shuffled_order():
    c = cases.get("cull")
    perm = cases.cull_permutation()
    sorted_cloud, shuffled = c["clouds"]
    assert np.array_equal(shuffled, sorted_cloud[perm])
    f = PL.host_frames(c["planes"], "score", 0.0)
    for p in PREFERS:
        got = cases.want("cull", p)
        a, b = per_scan("cull", got["instance"])
        assert np.array_equal(b, a[perm])  # the same permutation
        assert np.array_equal(got["points"][0], got["points"][1])
        assert got["points"][0, CULL["far"]] == 0
        assert (a >= 0).all()  # `around` contains the whole cloud
        corner = np.nonzero((sorted_cloud == 1).all(1))[0]
        assert len(corner) == 1 and corner[0] == 4 * B - 1
        assert PL.host_inside(sorted_cloud[corner], f["frames"][0, CULL["touch"]]).all()
    assert cases.want("cull", "score")["instance"][4 * B - 1] == CULL["touch"]  # score 0.8: only `far` is above
    # the sphere of `touch` reaches the bounding box of the last workgroup at exactly its radius
    last = sorted_cloud[3 * B:].astype(np.float64)
    centre = f["frames"][0, CULL["touch"], 2:5].astype(np.float64)
    gap = np.maximum(np.maximum(last.min(0) - centre, centre - last.max(0)), 0)
    assert np.sqrt((gap * gap).sum()) == f["reach"][0, CULL["touch"]]
    assert (a == CULL["around"]).sum() > 100 and len(np.unique(a)) > 4


@pytest.mark.parametrize("seed", cases.GEOMETRIC_SEEDS)
def test_the_geometric_builder_keeps_nine_points_in_ten_and_float64_agrees(seed):
    case = "geometric%d" % seed
    c = cases.get(case)
    for cloud, n in zip(c["clouds"], c["generated"]):
        assert len(cloud) >= 0.9 * n, (len(cloud), n)  # a condition of the builder, not a tolerance
    for s, cloud in enumerate(c["clouds"]):
        _, face = cases.float64_margin(cloud, c["planes"]["box"][s, :int(c["planes"]["count"][s])])
        assert face.min() >= cases.FACE_MARGIN
    for p in PREFERS:
        got = cases.want(case, p)["instance"]
        assert np.array_equal(got, cases.float64_labels(case, p))
        assert (got >= 0).mean() > 0.3 and len(np.unique(got)) > 20
    assert not np.array_equal(cases.want(case, "score")["instance"], cases.want(case, "smallest")["instance"])


def test_rows_past_count_do_not_matter():
    for case in ("sizes", "chunks"):
        c = cases.get(case)
        for garbage in cases.GARBAGE:
            dirty = cases.planes(case, garbage)
            assert not np.array_equal(dirty["box"], c["planes"]["box"], equal_nan=True)
            for p in PREFERS:
                got = PL.host_label_points(dirty, c["clouds"], p)
                for k, v in cases.want(case, p).items():
                    assert np.array_equal(got[k], v), (case, garbage, p, k)


def test_the_cases_cover_the_lists():
    sizes = cases.get("sizes")
    assert [len(x) for x in sizes["clouds"]] == [1, B - 1, B, B + 1, 3 * B + 1]
    assert sizes["planes"]["count"].tolist() == [0, 1, 3, 8, 5] and sizes["cap"] == sizes["K"] == 8  # 0, 1, cap, mixed
    got = cases.want("sizes", "score")
    assert (per_scan("sizes", got["instance"])[0] == -1).all() and not got["points"][0].any()  # no rows: all -1
    assert got["points"][1, 0] >= 1 and got["points"][3].sum() > 0 and got["points"][4].sum() > 0
    chunks = cases.get("chunks")
    assert chunks["planes"]["count"].tolist() == [CH - 1, CH, CH + 1, chunks["cap"]]
    assert chunks["layout"] == "tiled" and chunks["cap"] == cases.CHUNK_TILES * chunks["K"] and chunks["NC"] == 3
    eligible = (PL.host_frames(chunks["planes"])["rank"] != 0).sum(1)
    assert (eligible > CH // 2).all()
    for p in PREFERS:  # the last row of every scan owns point 0: rows CH - 2, CH - 1, CH (the second chunk) and cap - 1
        got = cases.want("chunks", p)
        for s, (rows, inst) in enumerate(zip(cases.CHUNK_ROWS, per_scan("chunks", got["instance"]))):
            assert inst[0] == rows - 1 and got["points"][s, rows - 1] >= 1, (p, s)
    for case in cases.CASES:
        for cols in (3, 6):
            clouds = cases.clouds(case, cols)
            assert all(x.shape[1] == cols and x.dtype == np.float32 for x in clouds)
            assert all(np.array_equal(x[:, :3], y) for x, y in zip(clouds, cases.get(case)["clouds"]))
    assert PL.LABEL_BLOCK == 256 and PL.LABEL_BOX_CHUNK == 256


# ------------------------------------------------------------------ label_points on the host path
@pytest.mark.parametrize("case", ["sizes", "chunks"])
def test_label_points_host_path_both_layouts(case, tmp_path):
    c = cases.get(case)
    store = SC.ScanStore(cases.clouds(case, 6), None, "scannet", names=c["names"])
    found = cases.found(case, cases.arena(case))
    assert isinstance(found, D.TiledDetections) == (case == "chunks")
    for p in PREFERS:
        labels = PL.label_points(found, store, prefer=p)
        want = cases.want(case, p)
        assert isinstance(labels, PL.PointLabels) and len(labels) == len(store)
        assert labels.instance.dtype == np.int32 and np.array_equal(labels.instance, want["instance"])
        assert np.array_equal(labels.semantic, want["semantic"]) and np.array_equal(labels.points, want["points"])
        assert labels.points.shape == (len(store), c["cap"]) and labels.frames.shape == (len(store), c["cap"], 8)
        assert np.array_equal(labels.frames, want["frames"], equal_nan=True)
        inst = per_scan(case, want["instance"])
        for i in (0, len(store) - 1, -1):
            one = labels[i]
            assert sorted(one) == ["instance", "points", "semantic"]
            assert np.array_equal(one["instance"], inst[i]) and np.array_equal(one["points"], want["points"][i])
        assert labels.by_name(c["names"][1])["instance"] is not None
        row = int(np.argmax(want["points"][-1]))
        assert np.array_equal(labels.points_of(-1, row), np.nonzero(inst[-1] == row)[0])
        with pytest.raises(IndexError):
            labels[len(store)]
        labels.save(str(tmp_path / p))
        for i, name in enumerate(c["names"]):
            z = np.load(str(tmp_path / p / (name + "_labels.npz")))
            assert sorted(z.files) == ["instance", "min_score", "points", "prefer", "semantic"]
            assert np.array_equal(z["instance"], inst[i]) and str(z["prefer"]) == p and float(z["min_score"]) == 0.0
            assert np.array_equal(z["points"], want["points"][i, :int(c["planes"]["count"][i])])


def test_refusals():
    c = cases.get("sizes")
    store = SC.ScanStore(c["clouds"], None, "scannet", names=c["names"])
    found = cases.found("sizes", cases.arena("sizes"))
    other = list(c["names"])
    other[2] = "elsewhere"
    with pytest.raises(ValueError, match=r"scan 2 is 'sizes_2' in the detections and 'elsewhere' in the store"):
        PL.label_points(found, SC.ScanStore(c["clouds"], None, "scannet", names=other))
    with pytest.raises(ValueError, match="5 scans of detections, 4 in the store"):
        PL.label_points(found, SC.ScanStore(c["clouds"][:4], None, "scannet", names=c["names"][:4]))
    with pytest.raises(ValueError, match="prefer"):
        PL.label_points(found, store, prefer="largest")
    for bad in (float("nan"), float("inf"), "high"):
        with pytest.raises(ValueError, match="min_score"):
            PL.label_points(found, store, min_score=bad)
    with pytest.raises(ValueError, match="ScanStore"):
        PL.label_points(found, c["clouds"])
    with pytest.raises(ValueError, match="Detections"):
        PL.label_points(c["planes"], store)
    broken = cases.found("sizes", cases.arena("sizes"))
    del broken.layout["box"]
    with pytest.raises(ValueError, match="count, cls, score and box"):
        PL.label_points(broken, store)
    broken = cases.found("sizes", cases.arena("sizes"))
    broken.layout["box"] = (broken.layout["box"][0], (5, 8, 6))
    with pytest.raises(ValueError, match="do not form"):
        PL.label_points(broken, store)
    broken = cases.found("sizes", cases.arena("sizes"))
    broken.K = D.MAX_K + 1
    with pytest.raises(ValueError, match="K = 1025"):
        PL.label_points(broken, store)
    with pytest.raises(ValueError, match="clouds"):
        PL.host_label_points(c["planes"], c["clouds"][:2])


def test_exports_and_constants():
    assert V.label_points is PL.label_points and V.host_label_points is PL.host_label_points
    assert V.PointLabels is PL.PointLabels
    L = importlib.import_module("3dioumatch_amd._lib")
    for name in ("scene_detections_frames", "scene_points_label", "scene_points_label_scratch_bytes"):
        assert name in L._LOADER_SIGNATURES and name not in L.EXPORTS and hasattr(L.lib, name)
    for S, cap in ((1, 1), (3, 256), (65535, 4096)):  # a host function
        assert PL.label_scratch_bytes(S, cap) == 16 * S * cap
    assert PL.label_scratch_bytes(0, 4) == PL.label_scratch_bytes(4, 0) == 0
    header = open(os.path.join(ROOT, "include", "point_labels_hip.h")).read()
    assert "#define LABEL_BLOCK %d " % PL.LABEL_BLOCK in header
    assert "#define LABEL_BOX_CHUNK %d " % PL.LABEL_BOX_CHUNK in header
    assert 1 <= PL.LABEL_BLOCK <= 1024  # at most 1024 points per workgroup


# ------------------------------------------------------------------ tools/detect.py
def _tool():
    spec = importlib.util.spec_from_file_location("tools_detect_labels", os.path.join(ROOT, "tools", "detect.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


EXISTING_DEFAULTS = {
    'inputs': [], 'checkpoint': None, 'dataset': 'scannet', 'num_point': None, 'use_color': False, 'no_height': False,
    'num_target': 256, 'conf_thresh': 0.05, 'nms_iou': 0.25, 'use_iou_for_nms': False, 'per_class_proposal': False,
    'opt_step': 0, 'opt_rate': 5e-4, 'batch_size': 8, 'out': None, 'device': 'cuda:0', 'synthetic': 0, 'seed': 0,
    'tile': None, 'overlap': 1.0, 'min_points': 1, 'seam_nms': False, 'seam': None, 'voxel': None, 'voxel_keep': None}


def test_detect_tool_label_flags_leave_every_default():
    tool = _tool()
    flags = vars(tool.parser().parse_args([]))
    new = {'labels': False, 'labels_prefer': None, 'labels_min_score': None}
    assert flags == dict(EXISTING_DEFAULTS, **new)
    plain = tool.parser().parse_args(["a.npy", "--out", "o"])
    assert tool.labeling(plain) is None and tool.voxeling(plain) is None and tool.tiling(plain) is None
    assert tool.labeling(tool.parser().parse_args(["a.npy", "--out", "o", "--labels"])) == ("score", 0.0)
    flags = tool.parser().parse_args(["a.npy", "--out", "o", "--labels", "--labels-prefer", "smallest",
                                      "--labels-min-score", "0.4", "--voxel", "0.05", "--tile", "8"])
    assert tool.labeling(flags) == ("smallest", 0.4) and tool.tiling(flags) == ((8.0, 8.0), 1.0, 1)
    with pytest.raises(SystemExit, match="go with --labels"):
        tool.labeling(tool.parser().parse_args(["a.npy", "--labels-prefer", "score"]))
    with pytest.raises(SystemExit, match="go with --labels"):
        tool.labeling(tool.parser().parse_args(["a.npy", "--labels-min-score", "0.1"]))
    with pytest.raises(SystemExit, match="goes with --out"):
        tool.labeling(tool.parser().parse_args(["a.npy", "--labels"]))
    for bad in ("nan", "inf"):
        with pytest.raises(SystemExit, match="finite"):
            tool.labeling(tool.parser().parse_args(["a.npy", "--out", "o", "--labels", "--labels-min-score", bad]))
    with pytest.raises(SystemExit):  # argparse's own: not one of the choices
        tool.parser().parse_args(["a.npy", "--labels", "--labels-prefer", "largest"])


def test_detect_tool_writes_labels_on_a_host_store(tmp_path):
    tool = _tool()
    c = cases.get("ownership")
    raw = SC.ScanStore(c["clouds"], None, "scannet", names=c["names"])
    found = cases.found("ownership", cases.arena("ownership"))
    flags = tool.parser().parse_args(["x.npy", "--out", str(tmp_path), "--labels", "--labels-prefer", "smallest",
                                      "--labels-min-score", str(cases.OWN_MIN_SCORE)])
    result = tool.write_labels(found, raw, tool.labeling(flags), flags.out)
    want = cases.want("ownership", "smallest", cases.OWN_MIN_SCORE)
    assert os.listdir(str(tmp_path)) == ["ownership_0_labels.npz"]
    z = np.load(str(tmp_path / "ownership_0_labels.npz"))
    assert np.array_equal(z["instance"], want["instance"]) and np.array_equal(z["semantic"], want["semantic"])
    assert np.array_equal(z["points"], want["points"][0, :cases.OWN_ROWS])
    assert str(z["prefer"]) == "smallest" and float(z["min_score"]) == cases.OWN_MIN_SCORE
    assert np.array_equal(result.instance, want["instance"])
