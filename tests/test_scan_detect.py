"""CPU tests of the label-free scan path: host_floor against the installed numpy's np.percentile, the
host batches of votenet/scan_data.py against the labeled loaders' host path, the host form of the
packing rule and Detections.as_map_cls against a plain Python listing, input validation, and the
flags of tools/detect.py."""
import importlib
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, load_pkg

load_pkg()
SC = importlib.import_module("3dioumatch_amd.votenet.scan_data")
SD = importlib.import_module("3dioumatch_amd.votenet.scannet_data")
SU = importlib.import_module("3dioumatch_amd.votenet.sunrgbd_data")
D = importlib.import_module("3dioumatch_amd.votenet.detect")
V = importlib.import_module("3dioumatch_amd.votenet")


def same_floor(got, want):
    """the same bits, apart from the sign of a zero"""
    got, want = np.float32(got), np.float32(want)
    return got == want and (got.tobytes() == want.tobytes() or got == 0)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ------------------------------------------------------------------ host_floor
def _cloud_z(g, n, kind):
    if kind == 0:
        return (g.standard_normal(n) * 1.5 + 0.3).astype(np.float32)           # mixed sign
    if kind == 1:
        return (np.round(g.standard_normal(n) * 64) / 64).astype(np.float32)   # ties, +-0.0 among them
    if kind == 2:
        return np.full(n, np.float32(g.standard_normal()), np.float32)         # all equal
    return (-np.abs(g.standard_normal(n)) - 0.01).astype(np.float32)           # only negative


def test_host_floor_is_numpy_percentile():
    g = np.random.default_rng(2024)
    sizes = [1, 2, 3, 101, 102, 203] * 20 + [200000, 199999]
    sizes += [int(np.exp(g.uniform(0, np.log(200000)))) for _ in range(2000)]
    assert max(sizes) == 200000 and len(sizes) >= 2000
    checked = 0
    for i, n in enumerate(sizes):
        z = _cloud_z(g, n, i % 4)
        got, want = SC.host_floor(z), np.percentile(z.astype(np.float32), 0.99)
        assert isinstance(got, np.float32) and want.dtype == np.float32
        assert same_floor(got, want), (n, i % 4, got, want)
        checked += 1
    assert checked >= 2000
    z64 = g.standard_normal(1000)  # float64 input is cast first
    assert same_floor(SC.host_floor(z64), np.percentile(z64.astype(np.float32), 0.99))


# ------------------------------------------------------------------ host_batch against the labeled loaders
N = 500
COUNTS = (700, 500, 300)  # n > N, n == N, n < N
COMBOS = [(c, h) for c in (False, True) for h in (False, True)]


@pytest.fixture(scope="module")
def scannet_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("scannet_scans"))
    names = ["scene%04d_00" % i for i in range(len(COUNTS))]
    for i, (name, n) in enumerate(zip(names, COUNTS)):
        SD.write_synthetic_scans(d, [name], num_points=n, instances=5, boxes=3, seed=10 + i)
    return d, names


@pytest.fixture(scope="module")
def sunrgbd_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("sunrgbd_scans"))
    names = ["%06d" % (i + 1) for i in range(len(COUNTS))]
    for i, (name, n) in enumerate(zip(names, COUNTS)):
        SU.write_synthetic_scans(d, [name], num_points=n, boxes=3, seed=20 + i, dtype=np.float32)
    return d, names


@pytest.mark.parametrize("use_color,use_height", COMBOS)
def test_host_batch_is_the_scannet_loaders_eval_batch(scannet_dir, use_color, use_height):
    d, names = scannet_dir
    scenes = SD.ScanNetScenes(d, names, None, use_color=use_color, use_height=use_height)
    labeled = SD.ScanNetLoader(scenes, V.scannet_config(), N, seed=7)
    store = SC.ScanStore.from_files([os.path.join(d, s + "_vert.npy") for s in names], None, "scannet")
    assert store.names == names and store.columns == 6
    for s in range(len(names)):
        assert same_floor(store.floor[s], scenes.floor[s])
    loader = SC.ScanLoader(store, N, use_color=use_color, use_height=use_height, seed=7)
    for ids, counter in (([0, 1, 2], 0), ([2, 0], 5), ([1], 9)):
        want = labeled.host_batch("eval", ids, counter=counter)
        got = loader.host_batch(ids, counter=counter)
        assert got["point_clouds"].dtype == np.float32
        assert got["point_clouds"].shape == (len(ids), N, 3 + 3 * use_color + use_height)
        assert np.array_equal(bits(got["point_clouds"]), bits(want["point_clouds"]))
        assert np.array_equal(got["scan_idx"], want["scan_idx"])
    idx = loader.host_draws([0, 1], 3)["idx"]
    assert len(set(idx[0])) == N and len(set(idx[1])) == N  # distinct when n >= N


@pytest.mark.parametrize("use_color,use_height", COMBOS)
def test_host_batch_is_the_sunrgbd_loaders_eval_batch(sunrgbd_dir, use_color, use_height):
    d, names = sunrgbd_dir
    scenes = SU.SunRgbdScenes(d, names, None, use_color=use_color, use_height=use_height)
    labeled = SU.SunRgbdLoader(scenes, V.sunrgbd_config(), N, seed=3)
    store = SC.ScanStore.from_files([os.path.join(d, s + "_pc.npz") for s in names], None, "sunrgbd")
    assert store.names == names
    loader = SC.ScanLoader(store, N, use_color=use_color, use_height=use_height, seed=3)
    for ids, counter in (([0, 1, 2], 1), ([2, 1], 4)):
        want = labeled.host_batch("eval", ids, counter=counter)
        got = loader.host_batch(ids, counter=counter)
        assert np.array_equal(bits(got["point_clouds"]), bits(want["point_clouds"]))
        assert np.array_equal(got["scan_idx"], want["scan_idx"])


def test_explicit_draws_and_xyz_only_from_a_colour_store():
    g = np.random.default_rng(0)
    clouds = SC.synthetic_clouds(2, 50, seed=1)
    store = SC.ScanStore(clouds, None, "scannet", names=["a", "b"])
    loader = SC.ScanLoader(store, 8, use_color=False, use_height=True)
    idx = g.integers(0, 50, (2, 8))
    got = loader.host_batch([1, 0], draws={"idx": idx})["point_clouds"]
    for r, s in enumerate((1, 0)):
        assert np.array_equal(got[r, :, 0:3], clouds[s][idx[r], 0:3])
        assert np.array_equal(got[r, :, 3], clouds[s][idx[r], 2] - store.floor[s])
    with pytest.raises(ValueError, match="out of range"):
        loader.host_batch([0, 1], draws={"idx": np.full((2, 8), 50)})
    with pytest.raises(ValueError, match="use_color"):
        SC.ScanLoader(SC.ScanStore([c[:, :3] for c in clouds], None), 8, use_color=True)
    with pytest.raises(ValueError, match="1..64"):
        loader.host_batch(np.zeros(65, np.int64))


# ------------------------------------------------------------------ validation
@pytest.mark.parametrize("bad,match", [
    (np.zeros(12, np.float32), "shape"),
    (np.zeros((2, 3, 3), np.float32), "shape"),
    (np.zeros((5, 2), np.float32), "2 columns"),
    (np.zeros((5, 4), np.float32), "4 columns"),
    (np.zeros((5, 5), np.float32), "5 columns"),
    (np.zeros((0, 3), np.float32), "0 points"),
])
def test_malformed_clouds_are_refused_by_name(bad, match):
    good = np.zeros((4, 3), np.float32)
    with pytest.raises(SD.SceneError, match=match) as e:
        SC.ScanStore([good, bad], None, names=["fine", "broken"])
    assert str(e.value).startswith("scan broken:")


def test_mixed_widths_nonfinite_and_missing_files_are_refused(tmp_path):
    three, six = np.zeros((4, 3), np.float32), np.zeros((4, 6), np.float32)
    with pytest.raises(SD.SceneError, match="scan wide: 6 columns"):
        SC.ScanStore([three, six], None, names=["narrow", "wide"])
    nan, inf = six.copy(), three.copy()
    nan[2, 4] = np.nan
    with pytest.raises(SD.SceneError, match=r"NaN or Inf.*: b \(1\), d \(1\)$"):
        inf6 = six.copy()
        inf6[0, 0] = -np.inf
        SC.ScanStore([six, nan, six, inf6], None, names=["a", "b", "c", "d"])
    with pytest.raises(SD.SceneError, match="missing"):
        SC.ScanStore.from_files([str(tmp_path / "nothing_vert.npy")], None)
    np.savez(str(tmp_path / "x.npz"), other=three)
    with pytest.raises(SD.SceneError, match="has no 'pc'"):
        SC.ScanStore.from_files([str(tmp_path / "x.npz")], None)
    with pytest.raises(SD.SceneError, match="no scans"):
        SC.ScanStore([], None)
    np.save(str(tmp_path / "y.npy"), np.arange(12.0).reshape(4, 3))  # float64: cast to float32
    np.savez(str(tmp_path / "z_pc.npz"), pc=np.arange(12.0).reshape(4, 3))
    store = SC.ScanStore.from_files([str(tmp_path / "y.npy"), str(tmp_path / "z_pc.npz")], None, "sunrgbd")
    assert store.names == ["y", "z"] and store.clouds[0].dtype == np.float32 and len(store) == 2


# ------------------------------------------------------------------ the packing rule and as_map_cls
def _hand_made(per_class):
    """four scenes of K = 12: nothing kept, everything kept, equal scores, a mix"""
    g = np.random.default_rng(5)
    B, K, C = 4, 12, 3
    keep = np.zeros((B, K), bool)
    keep[1] = True
    keep[2, [1, 4, 5, 9, 11]] = True
    keep[3] = g.random(K) < 0.5
    obj = g.random((B, K)).astype(np.float32)
    obj[2, [1, 5, 11]] = 0.625  # ties among kept proposals: proposal order decides
    obj[2, 4] = 0.625
    obj[2, 9] = 0.25
    obj[1, 3] = obj[1, 8]
    cls = g.integers(0, C, (B, K))
    sem = g.random((B, K, C)).astype(np.float32)
    score = (sem * obj[:, :, None]) if per_class else obj
    box = g.standard_normal((B, K, 7)).astype(np.float32)
    corners = g.standard_normal((B, K, 8, 3)).astype(np.float32)
    return keep, obj, cls, score, box, corners, C


@pytest.mark.parametrize("per_class", [False, True])
def test_host_pack_and_as_map_cls_against_a_plain_listing(per_class):
    keep, obj, cls, score, box, corners, C = _hand_made(per_class)
    B, K = keep.shape
    packed = D.host_pack(keep, obj, cls, score, box, corners)
    assert packed["count"].tolist() == [0, K, 5, int(keep[3].sum())]
    for b in range(B):
        order = sorted([j for j in range(K) if keep[b, j]], key=lambda j: (-float(obj[b, j]), j))
        c = len(order)
        assert packed["proposal"][b, :c].tolist() == order
        for r, j in enumerate(order):
            assert packed["cls"][b, r] == cls[b, j]
            assert np.array_equal(bits(packed["score"][b, r]), bits(score[b, j]))
            assert np.array_equal(bits(packed["box"][b, r]), bits(box[b, j]))
            assert np.array_equal(bits(packed["corners"][b, r]), bits(corners[b, j]))
        for plane in ("proposal", "cls", "score", "box", "corners"):
            assert not packed[plane][b, c:].any()
    assert packed["proposal"][2, :5].tolist() == [1, 4, 5, 11, 9]  # equal scores: proposal order

    # the flat arena of a run of B scans, as detect() fills it on the device
    NC = C if per_class else 0
    layout, words = D.arena_layout(B, K, NC)
    arena = np.zeros(words, np.float32)
    for plane, (at, shape) in layout.items():
        flat = np.ascontiguousarray(packed[plane]).reshape(-1)
        arena[at:at + flat.size] = flat.view(np.float32) if flat.dtype == np.int32 else flat
    found = D.Detections(arena, ["s%d" % b for b in range(B)], K, NC, C)
    assert len(found) == B and found.by_name("s2")["count"] == 5
    listing = found.as_map_cls()
    for b in range(B):
        js = np.nonzero(keep[b])[0]
        if per_class:
            want = [(ii, corners[b, j], score[b, j, ii]) for ii in range(C) for j in js]
        else:
            want = [(int(cls[b, j]), corners[b, j], score[b, j]) for j in js]
        assert len(listing[b]) == len(want)
        for (gc, gb, gs), (wc, wb, ws) in zip(listing[b], want):
            assert gc == wc and type(gc) is type(wc)
            assert np.array_equal(bits(gb), bits(wb)) and bits(gs) == bits(ws)
    assert listing[0] == []


def test_detections_save_writes_one_file_per_scan(tmp_path):
    keep, obj, cls, score, box, corners, C = _hand_made(True)
    B, K = keep.shape
    packed = D.host_pack(keep, obj, cls, score, box, corners)
    layout, words = D.arena_layout(B, K, C)
    arena = np.zeros(words, np.float32)
    for plane, (at, shape) in layout.items():
        flat = np.ascontiguousarray(packed[plane]).reshape(-1)
        arena[at:at + flat.size] = flat.view(np.float32) if flat.dtype == np.int32 else flat
    names = ["s%d" % b for b in range(B)]
    D.Detections(arena, names, K, C, C).save(str(tmp_path / "out"))
    for b, name in enumerate(names):
        with np.load(str(tmp_path / "out" / (name + ".npz"))) as f:
            c = int(f["count"])
            assert c == packed["count"][b] and f["box"].shape == (c, 7) and f["corners"].shape == (c, 8, 3)
            assert np.array_equal(f["proposal"], packed["proposal"][b, :c])


# ------------------------------------------------------------------ tools/detect.py
def _tool():
    spec = importlib.util.spec_from_file_location("tools_detect", os.path.join(ROOT, "tools", "detect.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_detect_tool_help_lists_the_flags(capsys):
    tool = _tool()
    with pytest.raises(SystemExit) as e:
        tool.main(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for flag in ("--checkpoint", "--dataset", "--num_point", "--use_color", "--no_height", "--num_target",
                 "--conf_thresh", "--nms_iou", "--use_iou_for_nms", "--per_class_proposal", "--opt_step",
                 "--opt_rate", "--batch_size", "--out", "--device", "--synthetic"):
        assert flag in text, flag


def test_detect_tool_refuses_a_checkpoint_of_another_width(tmp_path):
    tool = _tool()
    path = str(tmp_path / "checkpoint.tar")
    torch.save({"model_state_dict": {tool.FIRST_WEIGHT: torch.zeros(64, 3 + 4, 1, 1)}}, path)
    with pytest.raises(SystemExit) as e:  # trained with colour and height; the flags say height only
        tool.main(["--checkpoint", path, str(tmp_path / "a.npy")])
    assert "takes 4 feature channels, the flags give 1" in str(e.value) and "--use_color" in str(e.value)
    with pytest.raises(SystemExit) as e:
        tool.main(["--checkpoint", path, "--use_color", "--no_height", str(tmp_path / "a.npy")])
    assert "the flags give 3" in str(e.value)
    flags = tool.parser().parse_args(["--use_color", "x.npy"])
    tool.check_checkpoint({tool.FIRST_WEIGHT: torch.zeros(64, 7, 1, 1)}, flags)  # matching: accepted
    with pytest.raises(SystemExit, match="not a detector"):
        tool.check_checkpoint({}, flags)
