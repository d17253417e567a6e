"""CPU tests of the SUN RGB-D scene loader (votenet/sunrgbd_data.py): the host restatement against the
reference's own datasets (tests/golden/sunrgbd_data_ref.npz, make_sunrgbd_data_golden.py), batch
layout, input validation, splits, the two colour normalisations, and sunrgbd_config().

Bounds of the comparison with the reference (none of them is taken from what the code gives):
  integers, masks            exact
  float32 clouds' floats     1 float32 ulp (point_clouds, ema_point_clouds, center_label,
                             size_residual_label, rot_mat, rot_angle, scale)
  heading_residual_label     3e-8 absolute: one float32 ulp at the largest residual, pi / 12
  vote_label                 2e-6 absolute, all nine columns: coordinates are below 8 m, a float32
                             ulp there is at most 4.8e-7, a vote is a difference of two such numbers
  float64 clouds             point_clouds / ema_point_clouds within 2 float32 ulps of the scene's
                             largest |coordinate|: the float32 store rounds the input (0.5 ulp),
                             |cos| + |sin| <= sqrt(2) and a scale <= 1.15 amplify it, the output
                             rounding adds 0.5 ulp: below 1.4 ulp in all
"""
import importlib
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_pkg

load_pkg()
SD = importlib.import_module("3dioumatch_amd.votenet.sunrgbd_data")
SN = importlib.import_module("3dioumatch_amd.votenet.scannet_data")
V = importlib.import_module("3dioumatch_amd.votenet")

GOLD = np.load(os.path.join(GOLDEN, "sunrgbd_data_ref.npz"))
SCENES = [str(s) for s in GOLD["scan_names"]]
N = int(GOLD["num_points"])
# variant -> (batch kind, use_color, unlabeled row?, unlabeled_labels)
VARIANTS = {"lab": ("semi", True, False, False), "unl": ("semi", False, True, True),
            "unl_nolab": ("semi", True, True, False), "det_train": ("pretrain", False, False, False),
            "det_color": ("pretrain", True, False, False), "det_val": ("eval", False, False, False)}
CLOUD_KEYS = ("point_clouds", "ema_point_clouds")
ULP_KEYS = ("center_label", "size_residual_label", "rot_mat", "rot_angle", "scale")
EXACT_KEYS = ("heading_class_label", "size_class_label", "sem_cls_label", "box_label_mask",
              "vote_label_mask", "flip_x_axis", "flip_y_axis")


def write_scenes(d, names=SCENES):
    for s in names:
        np.savez(os.path.join(str(d), s + "_pc.npz"), pc=GOLD[s + "_pc"])
        np.save(os.path.join(str(d), s + "_bbox.npy"), GOLD[s + "_bbox"])
        np.savez(os.path.join(str(d), s + "_votes.npz"), point_votes=GOLD[s + "_votes"])


def within_ulp(got, want, ulps=1, key=""):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, key
    tol = ulps * np.spacing(np.maximum(np.abs(got), np.abs(want)))
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    bad = err > tol
    assert not bad.any(), "%s: %d values off by more than %d ulp, e.g. %r vs %r" % (
        key, bad.sum(), ulps, got[bad][:3], want[bad][:3])


def golden_draws(variant, scene):
    pre = "%s_%s_draw_" % (variant, scene)
    d = {"idx": GOLD[pre + "idx"][None]}
    for short, key in (("ema", "ema_idx"), ("u", "u"), ("u_color", "u_color"), ("u_point", "u_point")):
        if pre + short in GOLD.files:
            d[key] = GOLD[pre + short][None]
    return d


def loader_for(tmp_path, use_color, device=None):
    write_scenes(tmp_path)
    scenes = SD.SunRgbdScenes(str(tmp_path), SCENES, device, use_color=use_color, use_height=True)
    cfg = V.sunrgbd_config(mean_size_arr=GOLD["mean_size"])
    return SD.SunRgbdLoader(scenes, cfg, N, seed=5)


def batch_args(variant, i):
    kind, _, unl_row, labels = VARIANTS[variant]
    if kind == "semi":
        return kind, ([], [i]) if unl_row else ([i], []), labels
    return kind, ([i], None), False


def compare_to_golden(got, variant, scene, report=None):
    """Every output the reference returned for (variant, scene) against `got`, with the bounds of
    the module docstring; `report` collects the largest error per key (printed by the callers)."""
    pre = "%s_%s_" % (variant, scene)
    pc = GOLD[scene + "_pc"]
    f64_cloud = pc.dtype == np.float64
    coord_ulp = float(np.spacing(np.float32(np.abs(pc).max())))
    keys = [k[len(pre):] for k in GOLD.files if k.startswith(pre) and "_draw_" not in k]
    assert "point_clouds" in keys
    for key in keys:
        want = GOLD[pre + key]
        g = np.asarray(got[key])[0]
        assert g.shape == want.shape, key
        err = float(np.abs(g.astype(np.float64) - want.astype(np.float64)).max()) if g.size else 0.0
        if report is not None:
            report[key] = max(report.get(key, 0.0), err)
        if key in EXACT_KEYS:
            assert np.array_equal(g.astype(np.float64), want.astype(np.float64)), key
        elif key == "vote_label":
            assert want.shape[1] == 9
            np.testing.assert_allclose(g, want, rtol=0, atol=2e-6, err_msg=key)
        elif key == "heading_residual_label":
            np.testing.assert_allclose(g, want, rtol=0, atol=3e-8, err_msg=key)
        elif key in CLOUD_KEYS and f64_cloud:
            assert err <= 2 * coord_ulp, (key, err, coord_ulp)
        else:
            assert key in CLOUD_KEYS + ULP_KEYS, key
            within_ulp(g, want, key=key)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_host_path_reproduces_the_reference(tmp_path, variant):
    kind, use_color, unl_row, labels = VARIANTS[variant]
    loader = loader_for(tmp_path, use_color)
    report = {}
    for i, s in enumerate(SCENES):
        kind, (lab, unl), labels = batch_args(variant, i)
        got = loader.host_batch(kind, lab, unl, unlabeled_labels=labels, draws=golden_draws(variant, s))
        compare_to_golden(got, variant, s, report)
        assert got["scan_idx"].tolist() == [i]
        assert got["supervised_mask"].tolist() == [0 if unl_row else 1]
    print(variant, "largest |error| per key:", {k: "%.3g" % v for k, v in sorted(report.items())})


def test_golden_covers_the_cases():
    counts = [GOLD[s + "_pc"].shape[0] for s in SCENES]
    assert min(counts) < N <= max(counts)
    nbox = [GOLD[s + "_bbox"].shape[0] for s in SCENES]
    assert 0 in nbox and 64 in nbox
    assert {str(GOLD[s + "_pc"].dtype) for s in SCENES} == {"float32", "float64"}
    two = three = 0
    for s in SCENES:
        v = GOLD[s + "_votes"]
        assert np.abs(GOLD[s + "_pc"][:, 0:3]).max() < 8.0
        on = v[:, 0] > 0
        d12 = np.abs(v[:, 1:4] - v[:, 4:7]).sum(1) > 0
        d13 = np.abs(v[:, 1:4] - v[:, 7:10]).sum(1) > 0
        d23 = np.abs(v[:, 4:7] - v[:, 7:10]).sum(1) > 0
        three += int((on & d12 & d13 & d23).sum())
        two += int((on & d12 & ~(d13 & d23)).sum())
    assert two > 0 and three > 0
    flips = {float(GOLD[k][0]) > 0.5 for k in GOLD.files if k.endswith("_draw_u")}
    assert flips == {True, False}
    per = 2 * np.pi / 12
    for k in GOLD.files:  # no augmented heading within 1e-6 of a bin boundary
        if k.endswith("heading_residual_label"):
            mask = GOLD[k.replace("heading_residual_label", "box_label_mask")] > 0
            assert (np.abs(GOLD[k].astype(np.float64)[mask]) < per / 2 - 1e-6).all(), k
    sampled_votes = [GOLD["lab_%s_vote_label" % s] for s in SCENES]
    assert any((np.abs(v[:, 0:3] - v[:, 3:6]).sum(1) > 0).any() for v in sampled_votes)
    assert any(k.endswith("_draw_u_point") for k in GOLD.files)


def test_batch_layout_matches_the_synthetic_batches(tmp_path):
    loader = loader_for(tmp_path, False)
    cfg = V.sunrgbd_config()
    for kind, want in (("pretrain", V.make_batch(2, N, cfg)),
                       ("semi", V.make_semi_batch(2, 2, N, cfg)),
                       ("semi_labels", V.make_semi_batch(2, 2, N, cfg, unlabeled_labels=True))):
        if kind == "pretrain":
            got = loader.host_batch("pretrain", [0, 3])
        else:
            got = loader.host_batch("semi", [0, 3], [1, 2], unlabeled_labels=kind == "semi_labels")
        assert set(got) == set(want), kind
        for k, v in want.items():
            assert tuple(got[k].shape) == tuple(v.shape), (kind, k)
            assert str(got[k].dtype) == str(v.dtype).replace("torch.", ""), (kind, k)
    got = loader.host_batch("semi", [2, 0], [3, 1])
    assert got["scan_idx"].tolist() == [2, 0, 3, 1]
    assert got["supervised_mask"].tolist() == [1, 1, 0, 0]
    assert got["flip_y_axis"].tolist() == [0, 0, 0, 0]
    assert got["heading_class_label"].max() > 0 and got["heading_class_label"].max() < 12
    got = loader.host_batch("eval", [0, 1, 2])
    assert set(got) == set(V.make_batch(3, N, cfg))


def test_shared_pieces_are_the_scannet_loaders():
    core = importlib.import_module("3dioumatch_amd.votenet.scene_loader")
    scan = importlib.import_module("3dioumatch_amd.votenet.scan_data")
    for name in ("sample_indices", "epoch_plan", "feed", "eval_batches", "SceneError", "draw_key", "launch"):
        assert getattr(SD, name) is getattr(SN, name), name
        for module in (SD, SN, scan):
            assert getattr(module, name) is getattr(core, name), (module.__name__, name)
    assert SD.SunRgbdLoader.build is SN.ScanNetLoader.build is core.SceneLoader.build


def test_host_draws_are_a_pure_function_and_keyed_by_source_point(tmp_path):
    write_scenes(tmp_path)
    scenes = SD.SunRgbdScenes(str(tmp_path), SCENES, None, use_color=True, use_height=True)
    cfg = V.sunrgbd_config(mean_size_arr=GOLD["mean_size"])
    small, large = SD.SunRgbdLoader(scenes, cfg, 64, seed=2), SD.SunRgbdLoader(scenes, cfg, 200, seed=2)
    a, b = small.host_draws("pretrain", [0, 2], None, 9), large.host_draws("pretrain", [0, 2], None, 9)
    assert np.array_equal(a["u_point"], b["u_point"]) and np.array_equal(a["u_color"], b["u_color"])
    assert set(a) == {"idx", "u", "u_color", "u_point"}
    c = small.host_draws("pretrain", [0, 2], None, 10)
    assert not np.array_equal(a["u_point"], c["u_point"]) and not np.array_equal(a["idx"], c["idx"])
    # a sampled point's colour does not depend on N
    ba, bb = small.host_batch("pretrain", [0], None, 9), large.host_batch("pretrain", [0], None, 9)
    ia, ib = a["idx"][0], b["idx"][0]
    common, pa, pb = np.intersect1d(ia, ib, return_indices=True)
    assert common.size > 5
    assert np.array_equal(ba["point_clouds"][0][pa, 3:6], bb["point_clouds"][0][pb, 3:6])
    u = SD.point_uniforms(2, 9, 0, 5000)
    assert u.shape == (2, 5000) and 0.0 <= u.min() and u.max() < 1.0
    assert 0.25 < (u[1] <= 0.3).mean() < 0.35  # the 30 % colour drop


# ------------------------------------------------------------------ input validation
def _scene_files(d, name, n=50, boxes=3, cols=6, vote_rows=None, vote_cols=10, box_cols=8, cls=3):
    g = np.random.default_rng(0)
    np.savez(os.path.join(str(d), name + "_pc.npz"), pc=g.random((n, cols)).astype(np.float32))
    b = np.zeros((boxes, box_cols))
    b[:, 3:6] = 0.5
    b[:, -1] = cls
    np.save(os.path.join(str(d), name + "_bbox.npy"), b)
    np.savez(os.path.join(str(d), name + "_votes.npz"),
             point_votes=np.zeros((n if vote_rows is None else vote_rows, vote_cols)))


def test_input_errors_name_the_scan(tmp_path):
    d = str(tmp_path)
    for missing in ("_pc.npz", "_bbox.npy", "_votes.npz"):
        _scene_files(d, "000100")
        os.remove(os.path.join(d, "000100" + missing))
        with pytest.raises(SD.SceneError, match="000100.*missing.*" + missing):
            SD.read_scene(d, "000100")
    _scene_files(d, "000101", cols=2)
    with pytest.raises(SD.SceneError, match=r"000101: pc has shape \(50, 2\), expected \(n, >= 3\)"):
        SD.read_scene(d, "000101")
    _scene_files(d, "000102", cols=4)
    assert SD.read_scene(d, "000102")["cloud"].shape == (50, 4)  # xyz + height
    with pytest.raises(SD.SceneError, match=r"000102: pc has shape \(50, 4\), expected \(n, >= 6\)"):
        SD.read_scene(d, "000102", use_color=True)
    _scene_files(d, "000103", vote_rows=49)
    with pytest.raises(SD.SceneError, match=r"000103: 50 points but point_votes has shape \(49, 10\)"):
        SD.read_scene(d, "000103")
    _scene_files(d, "000104", vote_cols=9)
    with pytest.raises(SD.SceneError, match=r"000104: 50 points but point_votes has shape \(50, 9\)"):
        SD.read_scene(d, "000104")
    _scene_files(d, "000105", box_cols=7)
    with pytest.raises(SD.SceneError, match=r"000105: _bbox.npy has shape \(3, 7\), expected \(boxes, 8\)"):
        SD.read_scene(d, "000105")
    _scene_files(d, "000106", boxes=65)
    with pytest.raises(SD.SceneError, match="000106: 65 boxes"):
        SD.read_scene(d, "000106")
    _scene_files(d, "000107", cls=10)
    with pytest.raises(SD.SceneError, match="000107: box 0 has class 10"):
        SD.read_scene(d, "000107")
    _scene_files(d, "000108", cls=-1)
    with pytest.raises(SD.SceneError, match="000108: box 0 has class -1"):
        SD.read_scene(d, "000108")
    _scene_files(d, "000109", n=0)
    with pytest.raises(SD.SceneError, match="000109: 0 points"):
        SD.read_scene(d, "000109")
    _scene_files(d, "000110", boxes=64)
    s = SD.read_scene(d, "000110", use_color=True)
    assert s["boxes"].shape == (64, 8) and s["cloud"].shape == (50, 7) and s["votes"].shape == (50, 10)
    _scene_files(d, "000111", boxes=0)
    assert SD.read_scene(d, "000111")["boxes"].shape == (0, 8)
    with pytest.raises(SD.SceneError, match="no scans"):
        SD.SunRgbdScenes(d, [], None)


def test_floor_height_is_the_files_percentile(tmp_path):
    write_scenes(tmp_path)
    for s in SCENES:
        pc = GOLD[s + "_pc"]
        sc = SD.read_scene(str(tmp_path), s, use_color=False, use_height=True)
        floor = np.percentile(pc[:, 2], 0.99)
        assert sc["floor"] == float(floor)
        assert np.array_equal(sc["cloud"][:, 3], (pc[:, 2] - floor).astype(np.float32))
        assert sc["cloud"].dtype == np.float32 and sc["boxes"].dtype == np.float64


def test_split_helpers(tmp_path):
    train, val = tmp_path / "train", tmp_path / "val"
    train.mkdir()
    val.mkdir()
    for s in ("000005", "000001", "000003", "000009"):
        _scene_files(train, s)
    for s in ("000002", "000004"):
        _scene_files(val, s)
    assert SD.available_scans(str(train)) == ["000001", "000003", "000005", "000009"]
    lst = tmp_path / "lab.txt"
    lst.write_text("000003\n000007\n")
    assert SD.labeled_split(str(train), str(lst)) == ["000003"]
    assert SD.unlabeled_split(str(train), str(lst)) == ["000001", "000005", "000009"]
    lst.write_text("000003\n000007\n000001\n000011\n")  # as long as train: the unlabeled list is all of train
    assert SD.unlabeled_split(str(train), str(lst)) == ["000001", "000003", "000005", "000009"]
    assert SD.val_split(str(val)) == ["000002", "000004"]


def test_same_scan_labeled_and_unlabeled_colour_differ_by_256(tmp_path):
    loader = loader_for(tmp_path, True)
    draws = loader.host_draws("semi", [1], [1], 4)
    draws["idx"][1] = draws["idx"][0]
    draws["ema_idx"][1] = draws["ema_idx"][0]
    draws["u"][1] = draws["u"][0]
    b = loader.host_batch("semi", [1], [1], draws=draws)
    for key in ("point_clouds", "ema_point_clouds"):
        lab, unl = b[key][0], b[key][1]
        assert np.array_equal(lab[:, 0:3], unl[:, 0:3]) and np.array_equal(lab[:, 6], unl[:, 6])
        assert np.array_equal(lab[:, 3:6], unl[:, 3:6] * np.float32(256.0))
        assert np.abs(lab[:, 3:6]).max() > 0.1


def test_explicit_draw_bounds_are_checked_before_launch(tmp_path):
    loader = loader_for(tmp_path, False)
    n1 = int(loader.scenes.count[1])
    bad = np.zeros((1, N), np.int64)
    bad[0, 7] = n1
    with pytest.raises(ValueError, match="'idx' out of range"):
        loader.pretrain_batch([1], draws={"idx": bad, "u": np.zeros((1, 3))})
    bad[0, 7] = -1
    with pytest.raises(ValueError, match="'idx' out of range"):
        loader.pretrain_batch([1], draws={"idx": bad, "u": np.zeros((1, 3))})
    ema = np.full((1, N), n1, np.int64)
    with pytest.raises(ValueError, match="'ema_idx' out of range"):
        loader.semi_batch([1], [], draws={"idx": np.zeros((1, N)), "ema_idx": ema, "u": np.zeros((1, 3))})
    with pytest.raises(ValueError, match="'u_point' have shape"):
        loader.pretrain_batch([1], draws={"idx": np.zeros((1, N)), "u_point": np.zeros((1, 2, n1 - 1))})
    with pytest.raises(RuntimeError, match="no device copy"):
        loader.pretrain_batch([1], draws={"idx": np.full((1, N), n1 - 1), "u": np.zeros((1, 3))})


def test_synthetic_scans_have_oriented_boxes_and_distinct_votes(tmp_path):
    SD.write_synthetic_scans(str(tmp_path), ["000200"], num_points=3000, boxes=8, seed=4, dtype=np.float64)
    sc = SD.read_scene(str(tmp_path), "000200", use_color=True)
    assert np.load(os.path.join(str(tmp_path), "000200_pc.npz"))["pc"].dtype == np.float64
    v = sc["votes"]
    on = v[:, 0] > 0
    assert 0.5 < on.mean() < 0.95 and (v[~on] == 0).all()
    assert (np.abs(v[on, 1:4] - v[on, 4:7]).sum(1) > 0).any()
    target = sc["cloud"][on, 0:3] + v[on, 1:4]  # the first vote of a point lands on a box centre
    d = np.abs(target[:, None, :] - sc["boxes"][None, :, 0:3]).max(2).min(1)
    assert d.max() < 1e-5


def test_sunrgbd_config_unchanged_without_arguments():
    cfg = V.sunrgbd_config()
    want = np.random.default_rng(10).uniform(0.3, 1.8, (10, 3)).astype(np.float32)
    assert cfg.mean_size_arr.dtype == np.float32 and np.array_equal(cfg.mean_size_arr, want)
    assert (cfg.num_class, cfg.num_heading_bin, cfg.num_size_cluster) == (10, 12, 10)
    assert not hasattr(cfg, "mean_size_arr_f64")
    real = V.sunrgbd_config(mean_size_arr=GOLD["mean_size"])
    assert np.array_equal(real.mean_size_arr, GOLD["mean_size"].astype(np.float32))
    assert np.array_equal(real.mean_size_arr_f64, GOLD["mean_size"])
    with pytest.raises(ValueError):
        V.sunrgbd_config(mean_size_arr=np.zeros((18, 3)))
