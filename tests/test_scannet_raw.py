"""Raw ScanNet scans -> the preprocessed layout on the CPU: the PLY reader, the seg tables and the numpy
restatement (votenet/scannet_raw.py) against the reference's export and export_one_scan
(tests/golden/make_scannet_raw_golden.py), the host validation, ScanNetScenes.from_raw(device=None) and
the front end."""
import importlib
import json
import os
import runpy

import numpy as np
import pytest

from conftest import ROOT
from scannet_raw_cases import (R, SCANS, assert_same_export, materialise, max_points, ref, reference_export,
                               reference_one_scan)

SD = importlib.import_module("3dioumatch_amd.votenet.scannet_data")
SC = importlib.import_module("3dioumatch_amd.votenet.scan_data")
SL = importlib.import_module("3dioumatch_amd.votenet.scene_loader")
SceneError = SL.SceneError


@pytest.fixture(scope="module")
def raw(tmp_path_factory):
    scans, tsv = materialise(tmp_path_factory.mktemp("scannet_raw"))
    label_map = R.read_label_map(tsv)
    return {"scans": scans, "tsv": tsv, "label_map": label_map,
            "records": {s: R.read_raw_scan(scans, s, label_map) for s in SCANS}}


# ------------------------------------------------------------------ the PLY reader
@pytest.mark.parametrize("binary", [True, False], ids=["binary", "ascii"])
@pytest.mark.parametrize("colour", [True, False], ids=["rgb", "xyz"])
def test_ply_round_trip(tmp_path, binary, colour):
    g = np.random.default_rng(3)
    vert = np.concatenate([g.normal(size=(37, 3)) * 3, g.integers(0, 256, (37, 3))], 1).astype(np.float32)
    vert = vert if colour else vert[:, 0:3]
    path = str(tmp_path / "mesh.ply")
    R.write_ply(path, vert, binary=binary, faces=3)
    got = R.read_ply_vertices(path)
    assert got.dtype == np.float32 and got.shape == vert.shape
    assert np.array_equal(got.view(np.uint32), vert.view(np.uint32))


def _ply(path, header, body=b""):
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(body)
    return str(path)


def test_ply_type_names_other_elements_and_ignored_properties(tmp_path):
    """every type name and alias; a scalar element in front of the vertices is skipped; alpha, a normal
    and properties in another order are ignored; the faces behind are not read (they are cut off)"""
    types = [("char", "i1"), ("uchar", "u1"), ("short", "<i2"), ("ushort", "<u2"), ("int", "<i4"), ("uint", "<u4"),
             ("float", "<f4"), ("double", "<f8"), ("int8", "i1"), ("uint8", "u1"), ("int16", "<i2"),
             ("uint16", "<u2"), ("int32", "<i4"), ("uint32", "<u4"), ("float32", "<f4"), ("float64", "<f8")]
    names = ["p%d" % k for k in range(len(types))]
    names[7], names[6], names[14] = "x", "y", "z"  # double, float, float32
    names[1], names[9], names[3] = "red", "green", "blue"  # uchar, uint8, ushort
    table = np.zeros(5, np.dtype(list(zip(names, [t for _, t in types]))))
    g = np.random.default_rng(0)
    for n in names:
        table[n] = g.integers(0, 100, 5)
    table["x"] = [0.5, -1.25, 3.0, 1e-3, 7.0]
    camera = np.zeros(2, np.dtype([("a", "<f4"), ("b", "<i2")]))
    header = ["ply", "format binary_little_endian 1.0", "comment made by hand", "obj_info none",
              "element camera 2", "property float a", "property short b", "element vertex 5"]
    header += ["property %s %s" % (t, n) for (t, _), n in zip(types, names)]
    header += ["element face 1000", "property list uchar int vertex_indices", "end_header"]
    got = R.read_ply_vertices(_ply(tmp_path / "t.ply", header, camera.tobytes() + table.tobytes()))
    want = np.stack([table[c].astype(np.float32) for c in ("x", "y", "z", "red", "green", "blue")], 1)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    # ascii: an element with a list property in front is skipped line by line
    header = ["ply", "format ascii 1.0", "element edge 2", "property list uchar int v", "element vertex 2",
              "property float z", "property float y", "property float x", "end_header"]
    got = R.read_ply_vertices(_ply(tmp_path / "a.ply", header, b"2 0 1\n3 0 1 2\n1 2 3\n4 5 6.5\n"))
    assert np.array_equal(got, np.array([[3, 2, 1], [6.5, 5, 4]], np.float32))


def test_ply_errors_name_the_file(tmp_path):
    xyz = ["property float x", "property float y", "property float z"]
    body = np.arange(6, dtype="<f4").tobytes()
    cases = {
        "list.ply": (["ply", "format binary_little_endian 1.0", "element face 1",
                      "property list uchar int vertex_indices", "element vertex 2"] + xyz + ["end_header"], body),
        "big.ply": (["ply", "format binary_big_endian 1.0", "element vertex 2"] + xyz + ["end_header"], body),
        "noz.ply": (["ply", "format binary_little_endian 1.0", "element vertex 3"] + xyz[:2] + ["end_header"], body),
        "short.ply": (["ply", "format binary_little_endian 1.0", "element vertex 3"] + xyz + ["end_header"], body),
        "short_ascii.ply": (["ply", "format ascii 1.0", "element vertex 3"] + xyz + ["end_header"], b"1 2 3\n4 5 6\n"),
        "short_row.ply": (["ply", "format ascii 1.0", "element vertex 2"] + xyz + ["end_header"], b"1 2 3\n4 5\n"),
        "header.ply": (["ply", "format ascii 1.0", "element vertex 2"] + xyz, b""),
        "type.ply": (["ply", "format ascii 1.0", "element vertex 1", "property quad x", "end_header"], b"1\n"),
        "notply.ply": (["plx"], b""),
    }
    for name, (header, data) in cases.items():
        path = _ply(tmp_path / name, header, data)
        with pytest.raises(SceneError, match=name.replace(".", r"\.")):
            R.read_ply_vertices(path)
    with pytest.raises(SceneError, match="nowhere"):
        R.read_ply_vertices(str(tmp_path / "nowhere.ply"))


def test_label_map_is_the_references(raw, tmp_path):
    m = raw["label_map"]
    assert m["office chair"] == 5 and m["trash can"] == 39 and m["monitor"] == 40 and len(m) == 12
    assert R.read_label_map(raw["tsv"], "id", "nyu40id")[5] == 5  # integer-looking keys become ints
    with pytest.raises(SceneError, match="column"):
        R.read_label_map(raw["tsv"], "raw_category", "nyu41id")


# ------------------------------------------------------------------ the restatement against the reference
@pytest.mark.parametrize("name", ["sceneA", "sceneC", "sceneD"])
def test_exact_scans_equal_the_reference(raw, name):
    got = R.host_export_raw_scan(raw["records"][name])
    assert_same_export(got, reference_export(name), name)
    assert_same_export(got, reference_one_scan(name), name)
    [through] = R.export_raw_scans([raw["records"][name]], None)
    assert_same_export(through, got, name)


def test_box_counts_of_the_golden(raw):
    assert reference_export("sceneC")["bbox"].shape == (64, 7)
    assert reference_export("sceneD")["bbox"].shape == (0, 7)
    a = raw["records"]["sceneA"]
    assert len(a["groups"]) == 12 and len(set(g[1] for g in a["groups"])) == 9
    assert (a["seg_object"] == 0).sum() > 0  # unannotated segments


@pytest.mark.parametrize("name", SCANS)
def test_object_labels_are_the_references(raw, name):
    """export's unfiltered box table: row o carries object o's label where the object has a vertex"""
    rec, boxes = raw["records"][name], ref()["%s_export_bbox" % name]
    assert boxes.shape[0] == rec["object_label"].shape[0]
    seen = np.isin(np.arange(1, boxes.shape[0] + 1), ref()["%s_export_ins_label" % name])
    assert np.array_equal(boxes[seen, 6], rec["object_label"][seen].astype(np.float64))
    assert not boxes[~seen].any()


def test_realistic_scan_within_the_float32_rounding_of_the_reference(raw):
    rec = raw["records"]["sceneB"]
    got, want = R.host_export_raw_scan(rec), reference_export("sceneB")
    assert np.array_equal(got["ins_label"], want["ins_label"]) and got["ins_label"].dtype == np.uint32
    assert np.array_equal(got["sem_label"], want["sem_label"]) and got["sem_label"].dtype == np.uint32
    # what the golden was built to hold
    ins = want["ins_label"]
    assert (ins == 5).sum() == 0 and (ins == 7).sum() == 1  # an object without a vertex, one with one
    assert got["vert"].dtype == np.float32 and got["vert"].shape == want["vert"].shape
    assert np.array_equal(got["vert"][:, 3:], want["vert"][:, 3:])
    g, w = got["vert"][:, 0:3], want["vert"][:, 0:3]
    unequal = int((g != w).sum())
    print("sceneB: %d of %d aligned float32 coordinates differ from the reference's" % (unequal, g.size))
    assert (np.abs(g.astype(np.float64) - w.astype(np.float64)) <= np.spacing(np.abs(w))).all()
    assert got["bbox"].dtype == np.float64 and got["bbox"].shape == want["bbox"].shape
    assert np.array_equal(got["bbox"][:, 6], want["bbox"][:, 6])
    tol = 2.0 * float(np.spacing(np.float32(np.abs(w).max())))
    worst = float(np.abs(got["bbox"][:, 0:6] - want["bbox"][:, 0:6]).max())
    print("sceneB: boxes differ by at most %.3g (bound %.3g)" % (worst, tol))
    assert worst <= tol


def test_subsampled_scan(raw):
    rec, n, N = raw["records"]["sceneE"], 5000, max_points("sceneE")
    assert N == 2048
    choice = ref()["sceneE_choice"]
    got = R.host_export_raw_scan(rec, N, choice=choice)
    want = reference_one_scan("sceneE")
    assert_same_export(got, want, "sceneE")
    [through] = R.export_raw_scans([rec], None, N, choices={"sceneE": choice})
    assert_same_export(through, got, "sceneE")
    # the project's own draw: the un-subsampled output indexed by sample_indices
    whole = R.host_export_raw_scan(rec, n)
    for seed, index in ((0, 0), (5, 3)):
        idx = SL.sample_indices(seed, 0, index, SL.DRAW_STUDENT, n, N)
        assert idx.shape == (N,) and len(np.unique(idx)) == N and idx.min() >= 0 and idx.max() < n
        drawn = R.export_raw_scans([rec], None, N, seed=seed, first_index=index)[0]
        assert_same_export(drawn, {"vert": whole["vert"][idx], "ins_label": whole["ins_label"][idx],
                                   "sem_label": whole["sem_label"][idx], "bbox": whole["bbox"]}, "sceneE")
        full_ref = reference_export("sceneE")
        assert np.array_equal(drawn["ins_label"], full_ref["ins_label"][idx])
        assert np.array_equal(drawn["sem_label"], full_ref["sem_label"][idx])
    for bad in (np.arange(N) + n - N + 1, np.full(N, -1)):
        with pytest.raises(ValueError, match="out of range"):
            R.export_raw_scans([rec], None, N, choices={"sceneE": bad})
    with pytest.raises(ValueError, match="nothing is drawn"):
        R.export_raw_scans([raw["records"]["sceneA"]], None, choices={"sceneA": np.arange(1000)})


# ------------------------------------------------------------------ validation
def _tables(rec, label_map, seg=None, groups=None):
    return R.seg_tables(rec["name"], rec["seg"] if seg is None else seg, rec["groups"] if groups is None else groups,
                        label_map)


def test_table_validation_names_the_scan(raw):
    rec, m = raw["records"]["sceneA"], raw["label_map"]
    groups = list(rec["groups"])
    seg = rec["seg"].copy()
    seg[3] = -2
    with pytest.raises(SceneError, match="sceneA.*negative"):
        _tables(rec, m, seg=seg)
    for missing in (2, 10 ** 6, -1):  # between the ids, past the table, negative
        with pytest.raises(SceneError, match="sceneA.*no vertex carries"):
            _tables(rec, m, groups=groups[:1] + [(groups[1][0], groups[1][1], [missing])] + groups[2:])
    with pytest.raises(SceneError, match="sceneA.*'plant'.*label map"):
        _tables(rec, m, groups=[(groups[0][0], "plant", groups[0][2])] + groups[1:])
    with pytest.raises(SceneError, match="sceneA.*outside 1\\.\\.12"):
        _tables(rec, m, groups=[(12, groups[0][1], groups[0][2])] + groups[1:])
    with pytest.raises(SceneError, match="sceneA.*outside 1\\.\\.12"):
        _tables(rec, m, groups=[(-1, groups[0][1], groups[0][2])] + groups[1:])
    with pytest.raises(SceneError, match="sceneA.*share an objectId"):
        _tables(rec, m, groups=[(groups[1][0], groups[0][1], groups[0][2])] + groups[1:])
    with pytest.raises(SceneError, match="sceneA.*no list of segments"):
        _tables(rec, m, groups=[(groups[0][0], groups[0][1], [])] + groups[1:])
    many = [(o, "chair", [int(rec["seg"][0])]) for o in range(R.MAX_INSTANCES + 1)]
    with pytest.raises(SceneError, match="sceneA.*1025 objects.*MAX_INSTANCES"):
        _tables(rec, m, groups=many)
    _tables(rec, m, groups=many[:-1])  # MAX_INSTANCES objects are fine


def _rewrite(raw, tmp_path, name, **change):
    """scene `name` of the golden with one file changed: key -> f(text) -> text"""
    scans = str(tmp_path / "scans")
    src = os.path.join(raw["scans"], name)
    os.makedirs(os.path.join(scans, name))
    for k, suffix in R.SUFFIXES.items():
        with open(os.path.join(src, name + suffix), "rb") as f:
            data = f.read()
        if k in change:
            data = change[k](data)
        if data is not None:
            with open(os.path.join(scans, name, name + suffix), "wb") as f:
                f.write(data)
    return scans


def test_file_validation_names_the_scan(raw, tmp_path):
    m = raw["label_map"]

    def shorter(data):
        d = json.loads(data)
        d["segIndices"] = d["segIndices"][:-1]
        return json.dumps(d).encode()

    with pytest.raises(SceneError, match="sceneA: 1000 vertices but 999 segIndices"):
        R.read_raw_scan(_rewrite(raw, tmp_path / "a", "sceneA", seg=shorter), "sceneA", m)
    with pytest.raises(SceneError, match="sceneA.*axisAlignment"):
        R.read_raw_scan(_rewrite(raw, tmp_path / "b", "sceneA", meta=lambda d: b"numDepthFrames = 0\n"), "sceneA", m)
    with pytest.raises(SceneError, match="sceneA: missing .*aggregation"):
        R.read_raw_scan(_rewrite(raw, tmp_path / "c", "sceneA", agg=lambda d: None), "sceneA", m)
    with pytest.raises(SceneError, match="sceneA.*truncated"):
        R.read_raw_scan(_rewrite(raw, tmp_path / "d", "sceneA", mesh=lambda d: d[:4000]), "sceneA", m)
    scans = str(tmp_path / "e")
    rec = raw["records"]["sceneD"]
    R.write_raw_scan(scans, "sceneD", rec["vert"][:, 0:3], rec["seg"], [], rec["matrix"])
    with pytest.raises(SceneError, match="sceneD.*red green blue"):
        R.read_raw_scan(scans, "sceneD", m)
    # the scan's own folder may be given, and the label map as the tsv's path
    again = R.read_raw_scan(os.path.join(raw["scans"], "sceneB"), "sceneB", raw["tsv"])
    assert np.array_equal(again["seg_label"], raw["records"]["sceneB"]["seg_label"])


def test_a_scan_with_65_boxes_is_refused(raw):
    rec = dict(raw["records"]["sceneC"])
    groups = [(o, "chair" if label == "wall" and o == 5 else label, s) for o, label, s in rec["groups"]]
    rec["seg_label"], rec["seg_object"], rec["object_label"] = R.seg_tables("sceneC", rec["seg"], groups, raw["label_map"])
    with pytest.raises(SceneError, match="sceneC: 65 boxes, at most MAX_NUM_OBJ = 64"):
        R.host_export_raw_scan(rec)


# ------------------------------------------------------------------ the store, the files, the front end
def _assert_same_store(got, want):
    assert got.scan_names == want.scan_names and got.channels == want.channels
    for k in ("count", "offset", "nbox", "boxes", "ninst", "floor"):
        a, b = getattr(got, k), getattr(want, k)
        assert a.dtype == b.dtype and np.array_equal(a, b), k
    for a, b in zip(got.scenes, want.scenes):
        assert sorted(a) == sorted(b)
        for k in a:
            if isinstance(a[k], np.ndarray):
                assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
                assert a[k].tobytes() == b[k].tobytes(), k
            else:
                assert a[k] == b[k], k


@pytest.mark.parametrize("color,height", [(False, True), (True, False)])
def test_from_raw_on_the_host_is_the_store_of_its_export(raw, tmp_path, color, height):
    names = list(SCANS)
    store = SD.ScanNetScenes.from_raw(raw["scans"], names, raw["tsv"], None, use_color=color, use_height=height,
                                      max_points=2048, seed=4)
    assert store.count.tolist() == [1000, 2048, 1400, 1, 2048]
    out = str(tmp_path / "exported")
    store.export(out)
    assert sorted(os.listdir(out)) == sorted("%s_%s.npy" % (s, k) for s in names for k in
                                             ("vert", "ins_label", "sem_label", "bbox"))
    assert np.load(os.path.join(out, "sceneA_vert.npy")).dtype == np.float32
    assert np.load(os.path.join(out, "sceneA_ins_label.npy")).dtype == np.uint32
    assert np.load(os.path.join(out, "sceneD_bbox.npy")).shape == (0, 7)
    _assert_same_store(store, SD.ScanNetScenes(out, names, None, use_color=color, use_height=height))
    with pytest.raises(RuntimeError, match="from_raw"):
        SD.ScanNetScenes(out, names, None).export(str(tmp_path / "again"))
    with pytest.raises(SceneError, match="no scans"):
        SD.ScanNetScenes.from_raw(raw["scans"], [], raw["tsv"], None)


def test_read_scene_is_scene_from_arrays(tmp_path):
    SD.write_synthetic_scans(str(tmp_path), ["scene0000_00"], num_points=300, instances=5, boxes=3, seed=2)
    a = SD.read_scene(str(tmp_path), "scene0000_00", True, True)
    arrays = [np.load(str(tmp_path / ("scene0000_00_%s.npy" % k))) for k in ("vert", "ins_label", "sem_label", "bbox")]
    b = SD.scene_from_arrays("scene0000_00", *arrays, use_color=True, use_height=True)
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_scan_store_reads_ply(raw, tmp_path):
    vert = raw["records"]["sceneB"]["vert"]
    for cols, binary in ((6, True), (3, False)):
        R.write_ply(str(tmp_path / "cloud.ply"), vert[:, :cols], binary=binary, alpha=True)
        np.save(str(tmp_path / "cloud.npy"), vert[:, :cols])
        a = SC.ScanStore.from_files([str(tmp_path / "cloud.ply")], None)
        b = SC.ScanStore.from_files([str(tmp_path / "cloud.npy")], None)
        assert a.names == b.names == ["cloud"] and a.columns == cols
        assert a.clouds[0].tobytes() == b.clouds[0].tobytes() and np.array_equal(a.floor, b.floor)
    mesh = os.path.join(raw["scans"], "sceneA", "sceneA_vh_clean_2.ply")
    assert SC.ScanStore.from_files([mesh], None).clouds[0].tobytes() == raw["records"]["sceneA"]["vert"].tobytes()


def test_train_front_end_takes_raw_scans(raw, tmp_path):
    tool = runpy.run_path(os.path.join(ROOT, "tools", "train.py"))
    flags = tool["parser"]().parse_args(["--raw_scans", raw["scans"], "--label_map", raw["tsv"], "--meta_dir", "m"])
    assert flags.raw_scans == raw["scans"] and flags.label_map == raw["tsv"] and flags.data_dir is None
    with pytest.raises(SystemExit, match="--raw_scans DIR --label_map TSV"):
        tool["main"](["--stage", "pretrain", "--raw_scans", raw["scans"], "--meta_dir", str(tmp_path)])
    with pytest.raises(SystemExit, match="--raw_scans DIR --label_map TSV"):
        tool["main"](["--stage", "pretrain", "--raw_scans", raw["scans"], "--label_map", raw["tsv"],
                      "--data_dir", str(tmp_path), "--meta_dir", str(tmp_path)])
    # the split helpers take the scans' names from the raw folders as from the exported files
    (tmp_path / "scannetv2_train.txt").write_text("sceneB\nsceneX\nsceneA\n")
    assert SD.labeled_split(raw["scans"], str(tmp_path), "scannetv2_train.txt") == ["sceneB", "sceneA"]
    assert SD.available_scans(raw["scans"]) == list(SCANS)


def test_prepare_scannet_front_end(raw, tmp_path, capsys):
    tool = runpy.run_path(os.path.join(ROOT, "tools", "prepare_scannet.py"))
    names = tmp_path / "names.txt"
    names.write_text("sceneC\n\nsceneE\n")
    out = str(tmp_path / "out")
    tool["main"](["--scans", raw["scans"], "--label_map", raw["tsv"], "--out", out, "--names", str(names),
                  "--max_points", "2048", "--device", "cpu", "--seed", "9"])
    assert "sceneE: 2048 vertices, 8 boxes" in capsys.readouterr().out
    want = R.export_raw_scans([raw["records"][s] for s in ("sceneC", "sceneE")], None, 2048, seed=9)
    for s, w in zip(("sceneC", "sceneE"), want):
        assert_same_export({k: np.load(os.path.join(out, "%s_%s.npy" % (s, k))) for k in w}, w, s)
    assert R.raw_scan_names(raw["scans"]) == list(SCANS)
