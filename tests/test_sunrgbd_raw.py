"""Raw SUN RGB-D trainval folders on the CPU (votenet/sunrgbd_raw.py): the MAT reader against a foreign
writer's bytes and its own writer, its refusals, the numpy restatement against the reference's own
extraction (tests/golden/make_sunrgbd_raw_golden.py), the votes of a from_raw store, the exported folder
read back, the floor restatement against np.percentile, the refusals, and the two front ends' flags."""
import importlib
import os
import runpy

import numpy as np
import pytest

from sunrgbd_raw_cases import (FLOAT32, KEPT, R, SCENES, assert_same_bits, assert_same_export, materialise, num_point,
                               records, ref)

SUN = importlib.import_module("3dioumatch_amd.votenet.sunrgbd_data")
SC = importlib.import_module("3dioumatch_amd.votenet.scan_data")
SceneError = R.SceneError
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def raw(tmp_path_factory):
    folder = materialise(tmp_path_factory.mktemp("sunrgbd_raw"))
    return {"folder": folder, "records": dict(zip(SCENES, records(folder)))}


def by_kept_count():
    """The golden's scenes grouped by their kept count: [(num_point, names)]."""
    groups = {}
    for s in SCENES:
        groups.setdefault(num_point(s), []).append(s)
    return sorted(groups.items())


def recorded_choices(names):
    return {s: ref()[s + "_choice"] for s in names}


# ------------------------------------------------------------------ the MAT reader
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_reader_on_a_foreign_writers_bytes(tmp_path, tag):
    g = ref()
    path = str(tmp_path / "000123.mat")
    g["mat_%s_bytes" % tag].tofile(path)
    assert_same_bits(R.read_mat_points(path), g["mat_%s_array" % tag], tag)
    assert_same_bits(R.read_mat_points(path, "a", columns=None), np.arange(3.0).reshape(1, 3), "a")  # a small-form name


@pytest.mark.parametrize("compress", [True, False])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_reader_on_its_own_writer(tmp_path, compress, dtype):
    g = np.random.default_rng(5)
    array = np.concatenate([g.normal(size=(41, 3)), g.random((41, 3))], 1).astype(dtype)
    array[3, 2], array[4, 2] = -0.0, np.inf
    path = str(tmp_path / "000007.mat")
    R.write_mat(path, array, compress=compress)
    got = R.read_mat_points(path)
    assert got.flags["C_CONTIGUOUS"]
    assert_same_bits(got, array)
    # MATLAB stores integral values in the narrowest integer type; the reader converts to the class
    whole = np.round(array * 100).clip(-100, 100)
    whole[3, 2] = 0.0
    R.write_mat(path, whole, compress=compress, name="pc", storage=np.int8)
    assert_same_bits(R.read_mat_points(path, "pc"), whole)
    with pytest.raises(ValueError, match="survive"):
        R.write_mat(path, array[:3], storage=np.int16)
    sio = pytest.importorskip("scipy.io")
    R.write_mat(path, array, compress=compress)
    assert_same_bits(sio.loadmat(path)["instance"], array)
    R.write_mat(path, whole, compress=compress, name="pc", storage=np.int8)
    assert_same_bits(sio.loadmat(path, mat_dtype=True)["pc"], whole)  # (by default scipy returns the storage type)


def test_reader_refusals_name_the_scan(tmp_path):
    array = np.arange(24, dtype=np.float64).reshape(4, 6) / 7
    path = str(tmp_path / "000042.mat")

    def patched(offset, value):
        R.write_mat(path, array, compress=False)
        with open(path, "r+b") as f:
            f.seek(offset)
            f.write(value)

    # 128 header bytes, the matrix tag (8), the flags tag (8), then the flags word: class, flag bits
    patched(126, b"MI")
    with pytest.raises(SceneError, match="scan 000042: .*big-endian"):
        R.read_mat_points(path)
    patched(145, b"\x08")
    with pytest.raises(SceneError, match="scan 000042: .*complex"):
        R.read_mat_points(path)
    patched(144, b"\x05")
    with pytest.raises(SceneError, match="scan 000042: .*sparse"):
        R.read_mat_points(path)
    patched(144, b"\x09")  # int8
    with pytest.raises(SceneError, match="scan 000042: .*class 9"):
        R.read_mat_points(path)
    R.write_mat(path, array, name="points")
    with pytest.raises(SceneError, match="scan 000042: .*no variable 'instance' .*'points'"):
        R.read_mat_points(path)
    for compress in (True, False):
        R.write_mat(path, array, compress=compress)
        whole = open(path, "rb").read()
        for cut in (60, 130, len(whole) - 9):
            with open(path, "wb") as f:
                f.write(whole[:cut])
            with pytest.raises(SceneError, match="scan 000042: .*(truncated|not a Level-5)"):
                R.read_mat_points(path)
    R.write_mat(path, array[:, :5])
    with pytest.raises(SceneError, match="scan 000042: .*5 columns, expected 6"):
        R.read_mat_points(path)
    with pytest.raises(SceneError, match="scan 000043: missing"):
        R.read_mat_points(str(tmp_path / "000043.mat"))


# ------------------------------------------------------------------ the restatement against the reference
@pytest.mark.parametrize("name", SCENES)
def test_restatement_with_the_recorded_choice_is_the_references(raw, name):
    g = ref()
    rec = raw["records"][name]
    assert_same_bits(rec["points"], g[name + "_raw"], name)
    [got] = R.export_trainval([rec], None, num_point(name), choices=recorded_choices([name]))
    assert_same_bits(got["pc"], g[name + "_pc"], name + " pc")
    assert_same_bits(got["bbox"], g[name + "_bbox"], name + " bbox")
    assert got["pc"].dtype == (np.float32 if name in FLOAT32 else np.float64) and got["bbox"].dtype == np.float64
    # the store rows by read_scene's rule, written out: the file's dtype, one rounding
    pc = g[name + "_pc"]
    floor = np.percentile(pc[:, 2], 0.99)
    assert got["floor"] == floor and np.asarray(got["floor"]).dtype == pc.dtype
    want = np.concatenate([pc[:, 0:3], pc[:, 3:6] - 0.5, (pc[:, 2] - floor)[:, None]], 1)
    assert want.dtype == pc.dtype
    assert_same_bits(got["rows"], want.astype(np.float32), name + " rows")


def test_box_counts_and_dropped_classes_of_the_golden(raw):
    assert [raw["records"][s]["boxes"].shape[0] for s in SCENES] == [9, 0, 64, 2, 5, 4]
    lines = [len(bytes(ref()[s + "_label"]).decode().splitlines()) for s in SCENES]
    assert lines == [13, 2, 70, 2, 6, 5]  # the other classes' lines lie between the kept ones
    text = bytes(ref()["000003_label"]).decode().splitlines()
    assert text[0].split(" ")[0] not in R.TYPE2CLASS and text[1].split(" ")[0] in R.TYPE2CLASS


def test_the_projects_draw_has_both_branches(raw):
    a, b = raw["records"]["000001"], raw["records"]["000002"]
    got = R.export_trainval([a, b], None, 2048, seed=3, first_index=4)
    keep = R.sample_indices(3, 0, 4, R.DRAW_STUDENT, 2300, 2048)
    assert np.unique(keep).size == 2048  # n >= num_point: distinct
    assert_same_bits(got[0]["pc"], a["points"][keep])
    keep = R.sample_indices(3, 0, 5, R.DRAW_STUDENT, 150, 2048)
    assert np.unique(keep).size <= 150 and keep.max() < 150  # n < num_point: with replacement
    assert_same_bits(got[1]["pc"], b["points"][keep])
    assert R.NUM_POINT == 50000


# ------------------------------------------------------------------ the store
def test_votes_of_a_from_raw_store(raw, tmp_path):
    g = ref()
    for n, names in by_kept_count():
        store = SUN.SunRgbdScenes.from_raw(raw["folder"], names, None, use_color=True, use_height=True, num_point=n,
                                           choices=recorded_choices(names))
        assert store.votes == "boxes" and store.dev is None and store.count.tolist() == [n] * len(names)
        out = str(tmp_path / ("votes%d" % n))
        store.export_votes(out)
        for s, scene in zip(names, store.scenes):
            assert scene["votes"] is None and scene["cloud"].dtype == np.float32 and scene["cloud"].shape == (n, 7)
            rows = SUN.compute_votes(scene["cloud"], scene["boxes"])
            with np.load(os.path.join(out, s + "_votes.npz")) as f:
                assert_same_bits(f["point_votes"], rows.astype(np.float64), s + " votes")
            if s in FLOAT32:
                assert_same_bits(rows, g[s + "_votes"].astype(np.float32), s + " reference votes")
            else:
                # A float64 cloud is rounded to float32 before the vote is taken: not the reference's bits.
                # |coordinate| < 8, so the rounding moves a point by at most half an ulp there, 2^-22 = 2.4e-7
                # -- no point is within 1e-5 of a face (the maker's assertion), so the membership is the
                # reference's -- and the float32 vote, itself below 8, is rounded by as much again: 4.8e-7.
                assert np.array_equal(rows[:, 0], g[s + "_votes"][:, 0]), s
                assert np.allclose(rows, g[s + "_votes"], rtol=0, atol=1e-6), s


def _assert_same_store(a, b):
    assert a.scan_names == b.scan_names and a.channels == b.channels
    for k in ("count", "offset", "nbox", "boxes"):
        assert_same_bits(getattr(a, k), getattr(b, k), k)
    assert a.floor.dtype == b.floor.dtype == np.float64 and np.array_equal(a.floor, b.floor)  # ==: a zero's sign
    for x, y in zip(a.scenes, b.scenes):
        assert_same_bits(x["cloud"], y["cloud"], x["name"] + " cloud")
        assert_same_bits(x["boxes"], y["boxes"], x["name"] + " boxes")
        assert x["dtype"] == y["dtype"] and x["floor"] == y["floor"]


@pytest.mark.parametrize("color,height", [(False, True), (True, True), (True, False)])
def test_from_raw_on_the_host_is_the_store_of_its_exported_folder(raw, tmp_path, color, height):
    for n in KEPT:
        store = SUN.SunRgbdScenes.from_raw(raw["folder"], list(SCENES), None, use_color=color, use_height=height,
                                           num_point=n, seed=4)
        out = str(tmp_path / ("exported%d" % n))
        store.export(out)
        store.export_votes(out)
        assert sorted(os.listdir(out)) == sorted(s + k for s in SCENES for k in ("_pc.npz", "_bbox.npy", "_votes.npz"))
        with np.load(os.path.join(out, "000002_pc.npz")) as f:
            assert f["pc"].dtype == np.float64 and f["pc"].shape == (n, 6)
        assert np.load(os.path.join(out, "000002_bbox.npy")).shape == (0, 8)
        boxes = SUN.SunRgbdScenes(out, list(SCENES), None, use_color=color, use_height=height, votes="boxes")
        files = SUN.SunRgbdScenes(out, list(SCENES), None, use_color=color, use_height=height, votes="file")
        _assert_same_store(store, boxes)
        _assert_same_store(store, files)
        for x, y in zip(store.scenes, files.scenes):
            assert_same_bits(SUN.compute_votes(x["cloud"], x["boxes"]), y["votes"], x["name"] + " votes")
    with pytest.raises(RuntimeError, match="from_raw"):
        SUN.SunRgbdScenes(out, list(SCENES), None, votes="boxes").export(str(tmp_path / "again"))
    with pytest.raises(SceneError, match="no scans"):
        SUN.SunRgbdScenes.from_raw(raw["folder"], [], None)
    # an index list's path, data indices and names are one thing
    a = SUN.SunRgbdScenes.from_raw(raw["folder"], os.path.join(raw["folder"], "val_data_idx.txt"), None, num_point=64)
    b = SUN.SunRgbdScenes.from_raw(raw["folder"], [2, "4", "000006"], None, num_point=64)
    assert a.scan_names == b.scan_names == ["000002", "000004", "000006"]
    _assert_same_store(a, b)


# ------------------------------------------------------------------ the floor
def test_double_floor_restatement_is_np_percentile():
    g = ref()
    cases = [g[s + "_pc"][:, 2] for s in SCENES if s not in FLOAT32]
    cases += [g["000006_raw"][:, 2], np.zeros(5), -np.zeros(300), np.array([1.5]), np.array([-0.0, 0.0] * 80)]
    rng = np.random.default_rng(8)
    for n in (2, 3, 101, 102, 1977, 2048, 50000):
        cases.append(rng.normal(size=n))
        cases.append(np.round(rng.normal(size=n) * 4) / 4)  # long runs of equal values
    for z in cases:
        assert z.dtype == np.float64
        got = R.host_floor(z)
        assert got.dtype == np.float64 and got == np.percentile(z, 0.99), (z.shape, got)
    z = g["000006_pc"][:, 2]
    assert R.host_floor(z) == 0 and (z == 0).sum() > 100 and np.signbit(z[z == 0]).all()
    tie = g["000005_pc"][:, 2]
    assert tie.dtype == np.float32 and R.host_floor(tie) == np.percentile(tie, 0.99) == np.float32(-1.2578125)


def test_float32_floor_restatement_is_the_scan_stores():
    rng = np.random.default_rng(9)
    for n in (1, 2, 101, 1977, 2048, 50000):
        z = rng.normal(size=n).astype(np.float32)
        got = R.host_floor(z)
        assert got.dtype == np.float32
        assert_same_bits(got, SC.host_floor(z))
        assert got == np.percentile(z, 0.99)


# ------------------------------------------------------------------ refusals
def test_label_refusals_name_the_scan(raw, tmp_path):
    text = bytes(ref()["000001_label"]).decode().splitlines()
    kept = [l for l in text if l.split(" ")[0] in R.TYPE2CLASS]
    path = str(tmp_path / "000077.txt")

    def write(lines):
        with open(path, "w") as f:
            f.write("".join(l + "\n" for l in lines))

    write([kept[k % len(kept)] for k in range(64)] + [text[0]])
    assert R.read_labels(path).shape == (64, 8)
    write([kept[k % len(kept)] for k in range(65)])
    with pytest.raises(SceneError, match="scan 000077: 65 boxes, at most MAX_NUM_OBJ = 64"):
        R.read_labels(path)
    for bad, why in ((kept[0] + " 1.0", "14 fields"), (" ".join(kept[0].split(" ")[:12]), "12 fields"),
                     (kept[0].replace(" ", "  ", 1), "14 fields"), ("", "1 fields"),
                     (" ".join(kept[0].split(" ")[:12] + ["x"]), "could not convert")):
        write([kept[1], bad])
        with pytest.raises(SceneError, match="scan 000077: .* line 2 is malformed \\(.*%s" % why):
            R.read_labels(path)
    for word in ("nan", "inf", "-inf"):
        write([" ".join(text[0].split(" ")[:12] + [word])])  # in a line of a dropped class, too
        with pytest.raises(SceneError, match="scan 000077: .* line 1 holds NaN or Inf"):
            R.read_labels(path)
    write([])
    assert R.read_labels(path).shape == (0, 8) and R.read_labels(path).dtype == np.float64
    with pytest.raises(SceneError, match="scan 000078: missing"):
        R.read_labels(str(tmp_path / "000078.txt"))


def test_scene_refusals(raw, tmp_path):
    rec = dict(raw["records"]["000001"])
    rec["points"] = rec["points"].copy()
    rec["points"][7, 4] = np.nan
    rec["points"][9, 2] = np.inf
    with pytest.raises(SceneError, match=r"NaN or Inf .*000001 \(2\)"):
        R.export_trainval([raw["records"]["000003"], rec], None, 100)
    good = raw["records"]["000002"]
    for bad in (np.full(100, 150), np.full(100, -1)):
        with pytest.raises(ValueError, match="out of range"):
            R.export_trainval([good], None, 100, choices={"000002": bad})
    with pytest.raises(ValueError):
        R.export_trainval([good], None, 100, choices={"000002": np.zeros(99, np.int64)})
    with pytest.raises(ValueError, match="num_point >= 1"):
        R.export_trainval([good], None, 0)
    with pytest.raises(SceneError, match="scan 000009: missing"):
        R.read_trainval_scene(raw["folder"], 9)
    os.makedirs(str(tmp_path / "t" / "depth"))
    R.write_mat(str(tmp_path / "t" / "depth" / "000001.mat"), good["points"])
    with pytest.raises(SceneError, match="scan 000001: missing .*label_v1"):
        R.read_trainval_scene(str(tmp_path / "t"), "000001")
    with pytest.raises(SceneError, match="scan 000001: missing .*label.000001"):
        R.read_trainval_scene(str(tmp_path / "t"), "000001", use_v1=False)
    with pytest.raises(SceneError, match="integer data index"):
        R.read_trainval_scene(raw["folder"], "scene0000_00")
    with pytest.raises(SceneError, match="no such file"):
        R.read_idx_list(str(tmp_path / "nothing.txt"))
    over = dict(good, boxes=np.zeros((65, 8)))
    with pytest.raises(SceneError, match="scan 000002: 65 boxes"):
        R.export_trainval([over], None, 100)


# ------------------------------------------------------------------ the scan store and the front ends
def test_scan_store_reads_mat(raw, tmp_path):
    points = raw["records"]["000001"]["points"]
    for cols in (6, 3):
        R.write_mat(str(tmp_path / "000001.mat"), points[:, :cols])
        np.savez(str(tmp_path / "000001_pc.npz"), pc=points[:, :cols])
        a = SC.ScanStore.from_files([str(tmp_path / "000001.mat")], None, "sunrgbd")
        b = SC.ScanStore.from_files([str(tmp_path / "000001_pc.npz")], None, "sunrgbd")
        assert a.names == b.names == ["000001"] and a.columns == cols
        assert a.clouds[0].tobytes() == b.clouds[0].tobytes() and np.array_equal(a.floor, b.floor)


def test_synthetic_trainval_is_a_trainval_folder(tmp_path):
    names = R.synthetic_trainval(str(tmp_path), 5, points=400, boxes=6, seed=2, dtype=np.float64)
    assert names == ["000001", "000002", "000003", "000004", "000005"]
    assert R.read_idx_list(str(tmp_path / "train_data_idx.txt")) == names[:4]
    assert R.read_idx_list(str(tmp_path / "val_data_idx.txt")) == names[4:]
    rec = R.read_trainval_scene(str(tmp_path), 3)
    assert rec["points"].shape == (400, 6) and rec["points"].dtype == np.float64
    assert rec["boxes"].shape == (5, 8)  # one object in five is of a dropped class
    assert_same_bits(rec["boxes"], R.read_trainval_scene(str(tmp_path), 3, use_v1=False)["boxes"])
    votes = SUN.compute_votes(rec["points"].astype(np.float32), rec["boxes"])
    assert 0.3 < votes[:, 0].mean() < 0.9


def test_train_front_end_takes_sunrgbd(raw, tmp_path):
    tool = runpy.run_path(os.path.join(ROOT, "tools", "train.py"))
    flags = tool["parser"]().parse_args(["--dataset", "sunrgbd", "--raw_trainval", raw["folder"], "--use_sunrgbd_v2",
                                         "--votes", "boxes", "--val_dir", "v"])
    assert flags.dataset == "sunrgbd" and flags.raw_trainval == raw["folder"] and flags.use_sunrgbd_v2
    assert flags.votes == "boxes" and flags.val_dir == "v" and flags.data_dir is None
    base = tool["parser"]().parse_args([])
    assert base.dataset == "scannet" and base.votes == "file" and base.labeled_sample_list == "scannetv2_train.txt"
    assert base.raw_trainval is None and base.val_dir is None and not base.use_sunrgbd_v2
    sun = ["--dataset", "sunrgbd", "--stage", "pretrain"]
    for argv, message in (
            (sun + ["--raw_trainval", raw["folder"], "--data_dir", str(tmp_path)], "--raw_trainval DIR stands in place"),
            (sun + ["--raw_trainval", raw["folder"], "--val_dir", str(tmp_path)], "--raw_trainval DIR stands in place"),
            (sun + ["--data_dir", str(tmp_path)], "--data_dir and --val_dir, or --raw_trainval"),
            (sun + ["--data_dir", "a", "--val_dir", "b", "--use_sunrgbd_v2"], "--use_sunrgbd_v2 chooses"),
            (sun + ["--raw_scans", "a", "--label_map", "b"], "belong to --dataset scannet"),
            (["--dataset", "sunrgbd", "--stage", "semi", "--raw_trainval", raw["folder"]], "--labeled_sample_list"),
            (["--raw_trainval", raw["folder"], "--synthetic", "4"], "--raw_trainval belongs to --dataset sunrgbd"),
            (["--votes", "boxes", "--synthetic", "4"], "--votes belongs to --dataset sunrgbd")):
        with pytest.raises(SystemExit, match=message):
            tool["main"](argv)
    for argv in (sun + ["--raw_trainval", raw["folder"]], sun + ["--synthetic", "8"],
                 ["--dataset", "sunrgbd", "--stage", "semi", "--data_dir", "a", "--val_dir", "b", "--meta_dir", "m",
                  "--labeled_sample_list", "sunrgbd_v1_train_0.05.txt"]):
        flags = tool["parser"]().parse_args(argv)
        tool["check_dataset_flags"](flags, tool["settings"](flags))
    opt = tool["settings"](tool["parser"]().parse_args(["--dataset", "sunrgbd", "--stage", "semi"]))
    assert opt["labeled_batch"] == 4 and opt["unlabeled_batch"] == 8 and opt["num_target"] == 128  # the stage's defaults


def test_prepare_sunrgbd_front_end(raw, tmp_path, capsys):
    tool = runpy.run_path(os.path.join(ROOT, "tools", "prepare_sunrgbd.py"))
    out = str(tmp_path / "out")
    tool["main"](["--trainval", raw["folder"], "--split", "train", "--out", out, "--num_point", "1977",
                  "--device", "cpu", "--seed", "9", "--votes"])
    assert "000003: 1977 points (float32), 64 boxes" in capsys.readouterr().out
    train = SCENES[0::2]
    want = R.export_trainval([raw["records"][s] for s in train], None, 1977, seed=9)
    assert sorted(os.listdir(out)) == sorted(s + k for s in train for k in ("_pc.npz", "_bbox.npy", "_votes.npz"))
    for s, w in zip(train, want):
        with np.load(os.path.join(out, s + "_pc.npz")) as f:
            assert_same_bits(f["pc"], w["pc"], s)
        assert_same_bits(np.load(os.path.join(out, s + "_bbox.npy")), w["bbox"], s)
    store = SUN.SunRgbdScenes(out, list(train), None, use_color=True, votes="file")
    for scene, w in zip(store.scenes, want):
        assert_same_bits(scene["cloud"], w["rows"], scene["name"])
        assert_same_bits(scene["votes"], SUN.compute_votes(w["rows"], w["bbox"]), scene["name"])
    listed = tmp_path / "some.txt"
    listed.write_text("6\n\n2\n")
    tool["main"](["--trainval", raw["folder"], "--split", str(listed), "--out", str(tmp_path / "two"), "--num_point",
                  "64", "--device", "cpu"])
    assert sorted(os.listdir(str(tmp_path / "two"))) == ["000002_bbox.npy", "000002_pc.npz", "000006_bbox.npy",
                                                         "000006_pc.npz"]
    [w] = R.export_trainval([raw["records"]["000002"]], None, 64, first_index=1)  # keyed by its place in the list
    with np.load(str(tmp_path / "two" / "000002_pc.npz")) as f:
        assert_same_bits(f["pc"], w["pc"])
    assert_same_export(w, R.host_export_trainval_scene(raw["records"]["000002"], 64, 0, 1))
