"""The remove_empty_box / 2-D NMS additions on the MI355X: the point-count kernel
(csrc/box_points.hip) against the numpy closed form, exactly; the masked and 2-D modes of the NMS
kernels (csrc/lhs_nms.hip) against the host loop of tests/eval_empty_host.py; parse_predictions on
the reference's golden fully on the device; inference.evaluate with remove_empty_box switched on."""
import importlib
import math

import numpy as np
import pytest
import torch

import eval_empty_host as H
from conftest import golden, load_pkg

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _nms_mod():
    load_pkg()
    return importlib.import_module("3dioumatch_amd.votenet.pseudo_nms")


def _count_case(scenes, n, npts, pstride, seed):
    """boxes and points in a 6 m cube; box 0 holds every point, box 1 (n >= 2) none; points within
    1e-4 m of a face of a box of their scene are redrawn"""
    rng = np.random.default_rng(seed)
    center = rng.uniform(-3, 3, (scenes, n, 3)).astype(np.float32)
    size = rng.uniform(0.3, 2.5, (scenes, n, 3))
    heading = rng.uniform(-np.pi, np.pi, (scenes, n))
    center[:, 0], size[:, 0] = 0.0, 20.0
    if n >= 2:
        center[:, 1] = 50.0
    points = rng.uniform(-3, 3, (scenes, npts, pstride)).astype(np.float32)
    for _ in range(20):
        near = (H.face_margin(points, center, size, heading) < 1e-4).any(1)
        if not near.any():
            break
        points[near] = rng.uniform(-3, 3, (int(near.sum()), pstride)).astype(np.float32)
    assert not near.any()
    return points, center, size, heading


CHUNK = 512   # == pseudo_nms.BOX_POINT_CHUNK (asserted below): the sizes around one chunk


@pytest.mark.parametrize("pstride", [3, 4])
@pytest.mark.parametrize("npts", [1, 63, CHUNK - 1, CHUNK, CHUNK + 1, 4099])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("scenes", [1, 3])
def test_point_count_equals_the_closed_form(scenes, n, npts, pstride):
    P = _nms_mod()
    assert P.BOX_POINT_CHUNK == CHUNK
    points, center, size, heading = _count_case(scenes, n, npts, pstride, seed=scenes * 1000 + n + npts)
    want = H.count_closed_form(points, center, size, heading)
    assert (want[:, 0] == npts).all() and (n < 2 or (want[:, 1] == 0).all())
    d = [torch.from_numpy(a).to(DEV) for a in (points, center, size, heading)]
    count = torch.full((scenes, n), 7, dtype=torch.int32, device=DEV)
    got = P.box_point_count_gpu(*d, out=count)
    assert got.data_ptr() == count.data_ptr()
    first = count.cpu().numpy()
    P.box_point_count_gpu(*d, out=count)          # a second call into the same buffer: written,
    second = count.cpu().numpy()                  # not accumulated
    np.testing.assert_array_equal(first, want)
    np.testing.assert_array_equal(second, want)


def test_point_count_refuses_host_tensors_and_wrong_dtypes():
    P = _nms_mod()
    points, center, size, heading = (torch.from_numpy(a) for a in _count_case(1, 4, 16, 3, seed=1))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        P.box_point_count_gpu(points, center, size, heading)
    with pytest.raises(RuntimeError, match="float64"):
        P.box_point_count_gpu(points.to(DEV), center.to(DEV), size.float().to(DEV), heading.to(DEV))
    empty = P.box_point_count_gpu(points[:, :0].to(DEV), center.to(DEV), size.to(DEV), heading.to(DEV))
    assert empty.shape == (1, 4) and not empty.any()


def _nms_case(scenes, n, seed):
    """clumped boxes (so that many overlap), scores rounded to two digits (deliberate ties)"""
    rng = np.random.default_rng(seed)
    clumps = rng.uniform(-2.5, 2.5, (scenes, 8, 3))
    which = rng.integers(0, 8, (scenes, n))
    center = (np.take_along_axis(clumps, which[..., None].repeat(3, -1), 1) +
              rng.normal(0, 0.3, (scenes, n, 3))).astype(np.float32)
    size = rng.uniform(0.3, 1.6, (scenes, n, 3))
    heading = rng.uniform(-np.pi, np.pi, (scenes, n))
    score = np.round(rng.random((scenes, n)), 2).astype(np.float32)
    cls = rng.integers(0, 4, (scenes, n)).astype(np.int64)
    return center, size, heading, score, cls


def _valid_case(mode, scenes, n, rng):
    if mode == "none":
        return None
    if mode == "random":
        return (rng.random((scenes, n)) < 0.6).astype(np.int32)
    if mode == "one-scene-empty":
        v = (rng.random((scenes, n)) < 0.6).astype(np.int32)
        v[1] = 0
        return v
    v = np.zeros((scenes, n), np.int32)            # a single survivor per scene
    v[np.arange(scenes), rng.integers(0, n, scenes)] = 1
    return v


@pytest.mark.parametrize("mode", ["none", "random", "one-scene-empty", "single"])
@pytest.mark.parametrize("dims", [2, 3])
@pytest.mark.parametrize("n", [5, 64, 65, 256, 257, 1024])
def test_masked_nms_matches_the_host_loop(n, dims, mode):
    P = _nms_mod()
    scenes = 3
    center, size, heading, score, cls = _nms_case(scenes, n, seed=n * 10 + dims)
    valid = _valid_case(mode, scenes, n, np.random.default_rng(n + 7))
    d = [torch.from_numpy(a).to(DEV) for a in (center, size, heading, score, cls)]
    d_valid = None if valid is None else torch.from_numpy(valid).to(DEV)
    combos = [(False, False), (True, False)] if dims == 2 else [(False, False), (False, True), (True, True)]
    for old_type, same_class in combos:
        got = P.nms_aabb_masked_gpu(*d, 0.25, old_type, same_class, dims=dims, valid=d_valid).cpu().numpy()
        want = H.nms_masked_batch(center, size, heading, score, cls, 0.25, old_type, same_class, dims, valid)
        np.testing.assert_array_equal(got, want, err_msg="old_type=%s same_class=%s" % (old_type, same_class))
        if valid is not None:
            assert not got[valid == 0].any()
            assert (got.any(1) == valid.any(1)).all()     # all-invalid scene: all-zero row, else a winner
    if dims == 2:                                         # the 2-D mode does not read cls
        got = P.nms_aabb_masked_gpu(*d[:4], None, 0.25, False, False, dims=2, valid=d_valid).cpu().numpy()
        np.testing.assert_array_equal(
            got, H.nms_masked_batch(center, size, heading, score, None, 0.25, False, False, 2, valid))


@pytest.mark.parametrize("n", [64, 256, 1024])
def test_unmasked_3d_mode_is_the_plain_entry_point(n):
    P = _nms_mod()
    d = [torch.from_numpy(a).to(DEV) for a in _nms_case(3, n, seed=n + 1)]
    for old_type, same_class in ((False, False), (False, True), (True, True)):
        plain = P.nms3d_aabb_gpu(*d, 0.25, old_type, same_class)
        masked = P.nms_aabb_masked_gpu(*d, 0.25, old_type, same_class, dims=3, valid=None)
        ones = P.nms_aabb_masked_gpu(*d, 0.25, old_type, same_class, dims=3,
                                     valid=torch.ones(3, n, dtype=torch.int32, device=DEV))
        assert torch.equal(plain, masked) and torch.equal(plain, ones)


def test_masked_nms_refuses_what_it_cannot_serve():
    P = _nms_mod()
    d = [torch.from_numpy(a).to(DEV) for a in _nms_case(1, 8, seed=3)]
    with pytest.raises(RuntimeError, match="same-class"):
        P.nms_aabb_masked_gpu(*d, 0.25, False, True, dims=2)
    with pytest.raises(RuntimeError, match="dims"):
        P.nms_aabb_masked_gpu(*d, 0.25, False, False, dims=1)
    with pytest.raises(RuntimeError, match="valid"):
        P.nms_aabb_masked_gpu(*d, 0.25, False, False, dims=3, valid=torch.ones(1, 8, device=DEV))


@pytest.mark.parametrize("tag", H.VARIANTS)
def test_parse_predictions_matches_reference_on_the_device(tag):
    load_pkg()
    V = importlib.import_module("3dioumatch_amd.votenet")
    E = importlib.import_module("3dioumatch_amd.votenet.eval_helper")
    g = golden("eval_parse_empty_ref.npz")
    ep = H.inputs_of(g, DEV)
    config_dict = H.config_of(V, g, tag)
    if config_dict["remove_empty_box"]:
        size64, heading64 = E.decode_boxes(ep, config_dict["dataset_config"])
        count = E._count_points(ep["point_clouds"], ep["center"], size64, heading64)
        np.testing.assert_array_equal(count.cpu().numpy(), g["counts"])   # the reference's triangulation
    batch = E.parse_predictions(ep, config_dict)
    H.check_against_golden(g, tag, ep, batch, config_dict)


def test_evaluate_runs_with_remove_empty_box(monkeypatch):
    """inference.evaluate and iou_opt.evaluate hand `point_clouds` to parse_predictions unchanged:
    the count hook sees the batch's (B,N,4) cloud and the metrics are finite"""
    load_pkg()
    V = importlib.import_module("3dioumatch_amd.votenet")
    E = importlib.import_module("3dioumatch_amd.votenet.eval_helper")
    I = importlib.import_module("3dioumatch_amd.votenet.inference")
    O = importlib.import_module("3dioumatch_amd.votenet.iou_opt")
    step = importlib.import_module("3dioumatch_amd.votenet.step")
    data = importlib.import_module("3dioumatch_amd.votenet.data")
    cfg = V.scannet_config()
    det = step.build_detector(cfg, seed=0).to(DEV).eval()
    # enough objects that every class has ground truth: a class without any has recall 0 / 0, as in
    # the reference
    batches = [data.make_batch(4, 20000, cfg, seed=60, num_objects=40, device=DEV)]
    labelled = batches[0]["sem_cls_label"][batches[0]["box_label_mask"] == 1]
    assert len(set(labelled.tolist())) == cfg.num_class
    seen = []
    real = E._count_points

    def spy(points, center, size, heading):
        count = real(points, center, size, heading)
        seen.append((tuple(points.shape), torch.equal(points, batches[0]["point_clouds"]),
                     int((count >= 5).sum().item())))
        return count
    monkeypatch.setattr(E, "_count_points", spy)
    config_dict = {"dataset_config": cfg, "remove_empty_box": True, "use_3d_nms": True, "nms_iou": 0.25,
                   "use_old_type_nms": False, "cls_nms": True, "use_iou_for_nms": False,
                   "per_class_proposal": True, "conf_thresh": 0.05}
    for metrics in (I.evaluate(I.InferenceEngine(det), batches, config_dict),
                    O.evaluate(det, batches, config_dict)):
        assert len(metrics) == 2
        for m in metrics:
            assert all(math.isfinite(float(v)) for v in m.values()), m
    assert len(seen) == 2
    for shape, same, nonempty in seen:
        assert shape == (4, 20000, 4) and same
        assert nonempty > 0
