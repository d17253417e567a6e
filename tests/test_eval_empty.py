"""parse_predictions with `remove_empty_box` and the 2-D NMS branch (votenet/eval_helper.py) against
the REFERENCE's models/ap_helper.py:parse_predictions with its real extract_pc_in_box3d (vectors
from tests/golden/make_eval_empty_golden.py).  CPU: the two device hooks are replaced by the host
implementations of tests/eval_empty_host.py; pred_mask, nonempty_box_mask, list order, classes and
proposal indices identical, confidences within 2e-6 (the bound of test_eval_helper.py)."""
import importlib

import numpy as np
import pytest
import torch

import eval_empty_host as H
from conftest import golden, load_pkg


def host_hooks(E, monkeypatch):
    def count(points, center, size, heading):
        return torch.from_numpy(H.count_closed_form(points.cpu().numpy(), center.cpu().numpy(),
                                                    size.cpu().numpy(), heading.cpu().numpy())).to(center.device)

    def nms(center, size, heading, score, cls, thresh, old_type, same_class, dims, valid):
        out = H.nms_masked_batch(center.cpu().numpy(), size.cpu().numpy(), heading.cpu().numpy(),
                                 score.cpu().numpy(), cls.cpu().numpy(), thresh, old_type, same_class,
                                 dims, None if valid is None else valid.cpu().numpy())
        return torch.from_numpy(out).to(center.device)

    def no_plain_nms(*a, **k):
        raise AssertionError("the default branch's _nms3d was called for a masked / 2-D config")
    # raising=False: on code without the hooks the tests fail where it refuses the config
    monkeypatch.setattr(E, "_count_points", count, raising=False)
    monkeypatch.setattr(E, "_nms_masked", nms, raising=False)
    monkeypatch.setattr(E, "_nms3d", no_plain_nms)


@pytest.mark.parametrize("tag", H.VARIANTS)
def test_parse_predictions_matches_reference_with_host_hooks(tag, monkeypatch):
    load_pkg()
    V = importlib.import_module("3dioumatch_amd.votenet")
    E = importlib.import_module("3dioumatch_amd.votenet.eval_helper")
    g = golden("eval_parse_empty_ref.npz")
    host_hooks(E, monkeypatch)
    ep = H.inputs_of(g, torch.device("cpu"))
    config_dict = H.config_of(V, g, tag)
    batch = E.parse_predictions(ep, config_dict)
    H.check_against_golden(g, tag, ep, batch, config_dict)


def test_host_count_equals_the_reference_triangulation():
    """the closed-form test in float32 == Delaunay(corners).find_simplex(p) >= 0 on the golden, whose
    generator keeps every point 1e-4 m from every face; both sides of the `< 5` threshold occur"""
    load_pkg()
    V = importlib.import_module("3dioumatch_amd.votenet")
    E = importlib.import_module("3dioumatch_amd.votenet.eval_helper")
    g = golden("eval_parse_empty_ref.npz")
    ep = H.inputs_of(g, torch.device("cpu"))
    size64, heading64 = E.decode_boxes(ep, V.sunrgbd_config())
    got = H.count_closed_form(g["in::point_clouds"], g["in::center"], size64.numpy(), heading64.numpy())
    np.testing.assert_array_equal(got, g["counts"])
    assert {3, 4, 5, 6} <= set(g["counts"].ravel().tolist())
    assert (g["counts"] >= 5).any(1).all()
    assert 0.02 <= (g["counts"] < 5).mean() <= 0.5
    margin = H.face_margin(g["in::point_clouds"], g["in::center"], size64.numpy(), heading64.numpy())
    assert margin.min() >= 1e-4


def test_default_config_still_calls_the_plain_nms_only(monkeypatch):
    """both keys at their defaults: _nms3d and nothing else, as before"""
    load_pkg()
    V = importlib.import_module("3dioumatch_amd.votenet")
    E = importlib.import_module("3dioumatch_amd.votenet.eval_helper")
    g = golden("eval_parse_empty_ref.npz")
    calls = []

    def plain(center, size, heading, score, cls, thresh, old_type, same_class):
        calls.append("nms3d")
        return torch.ones(score.shape, dtype=torch.bool)

    def never(*a, **k):
        raise AssertionError("a new hook was called for the default config")
    monkeypatch.setattr(E, "_nms3d", plain)
    monkeypatch.setattr(E, "_count_points", never, raising=False)
    monkeypatch.setattr(E, "_nms_masked", never, raising=False)
    ep = H.inputs_of(g, torch.device("cpu"))
    del ep["point_clouds"]          # the default branch does not need the cloud
    config_dict = {"dataset_config": V.sunrgbd_config(), "nms_iou": 0.25, "conf_thresh": 0.05,
                   "use_old_type_nms": False, "cls_nms": True, "use_iou_for_nms": False,
                   "per_class_proposal": False}
    E.parse_predictions(ep, config_dict)
    assert calls == ["nms3d"] and "nonempty_box_mask" not in ep


def test_host_masked_nms_equals_nms_on_the_subset():
    """the property the kernels' mask relies on: masking == running on boxes[valid == 1]"""
    rng = np.random.default_rng(5)
    n = 90
    lo = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    aabb = np.concatenate([lo, lo + rng.uniform(0.3, 1.5, (n, 3)).astype(np.float32)], 1)
    score = np.round(rng.random(n), 1).astype(np.float32)      # ties
    cls = rng.integers(0, 3, n)
    valid = (rng.random(n) < 0.6).astype(np.int32)
    idx = np.nonzero(valid)[0]
    for dims in (2, 3):
        for same_class in ((False,) if dims == 2 else (False, True)):
            got = H.nms_masked(aabb, score, cls, 0.25, False, same_class, dims, valid)
            sub = H.nms_masked(aabb[idx], score[idx], cls[idx], 0.25, False, same_class, dims, None)
            want = np.zeros(n, bool)
            want[idx[sub]] = True
            assert np.array_equal(got, want)


def test_new_symbols_are_exported_and_bound():
    import ctypes
    load_pkg()
    L = importlib.import_module("3dioumatch_amd._lib")
    for name, nargs in (("lhs_box_point_count", 10), ("lhs_nms_aabb_masked", 14)):
        assert name in L.EXPORTS
        fn = getattr(L.lib, name)
        assert len(fn.argtypes) == nargs and fn.restype is ctypes.c_int
    # non-positive sizes return 0 without a launch (no device needed)
    assert L.lib.lhs_box_point_count(0, 4, 4, 3, None, None, None, None, None, None) == 0
    assert L.lib.lhs_box_point_count(2, 0, 4, 3, None, None, None, None, None, None) == 0
    assert L.lib.lhs_box_point_count(2, 4, 0, 3, None, None, None, None, None, None) == 0
    assert L.lib.lhs_nms_aabb_masked(0, 4, None, None, None, None, None, 0.25, 0, 0, 2, None, None, None) == 0
    # the 2-D mode has no same-class form; dims is 2 or 3
    assert L.lib.lhs_nms_aabb_masked(1, 4, None, None, None, None, None, 0.25, 0, 1, 2, None, None, None) != 0
    assert L.lib.lhs_nms_aabb_masked(1, 4, None, None, None, None, None, 0.25, 0, 0, 4, None, None, None) != 0
