"""The test-time criterion on the MI355X: the eval kernels of csrc/votenet_loss.hip (eval_decode_kernel,
eval_terms_kernel, eval_stats_kernel) through the C ABI (votenet_eval_loss_decode, votenet_eval_loss) and the
binding's pass builder, the running sums, the public get_loss and both evaluate(..., with_loss=True).

  * the kernels against the float64 truth of tests/eval_loss_cases.py (models/loss_helper.py:25-291 written from its
    formulas) at the shapes of loss_kernel_cases.CASES -- each the smallest at which a path exists: `second_block`
    (5, 300, 70, 300: a partial proposal block, 25 partial rows), `one_lane_over` (3, 257, 64, 257, two votes per
    seed), `limits_wide_rows` (2, 513, 256, 40; NH = 33, NS = 40, NC = 37, one IoU channel), `k_limit` (1, 2048, 1,
    1), `smallest`, `workload_block` -- and a case without a positive (cnt = 0, every vote mask zero: every masked
    term exactly 0).  Strided head outputs (the detector's transposed slices) and contiguous ones, as the cases
    say.  Statistics within BOUND * max(1, |ref|), BOUND = 1e-5 as tests/test_loss_kernels.py derives it (a
    schedule error moves a statistic by 1e-3 or more); labels, masks and assignments equal; the decoded boxes
    within one rounding per operation.
  * two runs give the same bits.
  * accum: three different batches through one accumulator equal the three statistics vectors added in that order
    in fp32, bit for bit; accum = NULL gives the same statistics and touches nothing else.
  * fused_loss.get_loss_fused against losses.get_loss with the fused path off on the reference's seeded eval batch
    (tests/golden/eval_loss_ref.npz): the 20 keys within 1e-5 * max(1, |ref|) (two fp32 evaluations of the same
    formulas, each measured below 5e-7 of float64), labels equal, iou_labels and pred_bbox within 1e-6 (the same
    IoU kernel on boxes decoded by the same two operations).
  * end to end with a small detector and the synthetic batches of tests/test_inference_gpu.py:
    evaluate(engine, ..., with_loss=True, device_ap=True) gives the metrics of with_loss=False exactly and the
    plain mean of per-batch losses.get_loss on the plain eval forward within 1e-4 * max(1, |ref|) (that file's
    forward tolerance); iou_opt.evaluate(..., opt_step=2, with_loss=True) moves center_loss.

Measured on the MI355X against float64, |err| / max(1, |ref|), worst statistic per case, the fp32 tensor formulation
(losses.get_loss, fused path off) / the kernels:
  workload_block 8.1e-8 / 8.1e-8 (size_cls_loss); second_block 8.3e-8 (sem_cls_loss) / 7.8e-8 (heading_cls_loss);
  one_lane_over 1.5e-7 / 1.5e-7 (detection_loss); limits_wide_rows 6.9e-8 (size_cls_loss) / 7.5e-8
  (heading_cls_loss); k_limit 1.9e-7 / 1.9e-7 (vote_loss); smallest 4.7e-8 (iou_acc_obj) / 6.2e-8 (size_reg_loss);
  one_lane_over without a positive 2.0e-8 (detection_loss) / 3.6e-8 (iou_acc).
No case exceeds 5e-7, so every case keeps the bound of 1e-5.  Labels, masks and assignments equal everywhere.
"""
import importlib
import math

import numpy as np
import pytest
import torch

import eval_loss_cases as cases
from conftest import load_pkg
from loss_kernel_cases import CASES
from test_eval_loss import (LABELS, _modules, check_case, check_plants, golden_end_points, run_case)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BOUND = {name: 1e-5 for name in CASES}


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def _kernel_case(name, no_positive, monkeypatch, accum=None):
    _, _, fused = _modules()
    c, ref = cases.build(name, no_positive), cases.reference(name, no_positive)
    check_plants(c, ref)
    return c, ref, run_case(fused, DEV, c, monkeypatch, accum)


@pytest.mark.parametrize("name", list(CASES))
def test_kernels_against_float64(name, monkeypatch):
    c, ref, out = _kernel_case(name, False, monkeypatch)
    check_case(c, ref, out, name, BOUND[name])
    _, _, again = _kernel_case(name, False, monkeypatch)
    for key in ("stats", "objectness_mask", "boxes", "gt_boxes"):
        assert np.array_equal(_bits(out[key]), _bits(again[key])), (name, key, "two runs differ")
    for key in ("objectness_label", "object_assignment"):
        assert np.array_equal(out[key], again[key]), (name, key)


def test_kernels_no_positive_anywhere(monkeypatch):
    c, ref, out = _kernel_case("one_lane_over", True, monkeypatch)
    check_case(c, ref, out, "one_lane_over no-positive", BOUND["one_lane_over"])
    st = dict(zip(cases.STAT_KEYS, out["stats"]))
    for key in ("vote_loss", "heading_cls_loss", "heading_reg_loss", "size_cls_loss", "size_reg_loss", "sem_cls_loss",
                "iou_loss", "cls_acc_obj", "pred_iou_obj_value", "iou_acc_obj", "pos_ratio", "obj_count"):
        assert st[key] == 0.0, key


def test_accumulator_adds_in_order_bit_exactly(monkeypatch):
    _, _, fused = _modules()
    names = ("second_block", "smallest", "one_lane_over")
    alone = [_kernel_case(n, False, monkeypatch)[2]["stats"] for n in names]
    accum = torch.zeros(fused.EV_COUNT, dtype=torch.float32, device=DEV)
    guard = torch.full((fused.EV_COUNT + 128,), -12345.678, dtype=torch.float32, device=DEV)
    inside = guard[64:64 + fused.EV_COUNT]
    inside.zero_()
    want = np.zeros(fused.EV_COUNT, np.float32)
    for n, stats in zip(names, alone):
        got = _kernel_case(n, False, monkeypatch, accum)[2]["stats"]
        assert np.array_equal(_bits(got), _bits(stats)), (n, "the statistics depend on accum")
        _kernel_case(n, False, monkeypatch, inside)
        want = (want + stats).astype(np.float32)
        assert np.array_equal(_bits(accum.cpu().numpy()), _bits(want)), n
    assert np.array_equal(_bits(inside.cpu().numpy()), _bits(want))
    host = guard.cpu().numpy()
    assert (host[:64] == np.float32(-12345.678)).all() and (host[64 + fused.EV_COUNT:] == np.float32(-12345.678)).all()
    assert want[fused.EV_OBJ_COUNT] == sum(s[fused.EV_OBJ_COUNT] for s in alone) > 0


def test_entry_points_reject_shapes_beyond_the_limits(monkeypatch):
    """G = 257 and K = 2049 are refused before anything is launched (hipErrorInvalidValue), as by the training
    entry points; so is a missing partials / stats buffer"""
    import ctypes
    _, _, fused = _modules()
    L = importlib.import_module("3dioumatch_amd._lib")
    seen = {}
    real = fused._launch_eval
    monkeypatch.setattr(fused, "_launch_eval", lambda name, a, dev, *more: (seen.update({name: (a, more)}),
                                                                            real(name, a, dev, *more)))
    run_case(fused, DEV, cases.build("smallest"), monkeypatch)
    a, (stats, _) = seen["votenet_eval_loss"]
    stream = L.current_stream_ptr(DEV)
    stats_before = stats.clone()
    for change in (dict(G=257), dict(K=2049), dict(NI=0), dict(partials=None)):
        b = type(a).from_buffer_copy(a)
        for field, value in change.items():
            setattr(b, field, value)
        assert L.lib.votenet_eval_loss(ctypes.byref(b), ctypes.c_void_p(stats.data_ptr()), None, stream) == 1, change
        if "partials" not in change:
            assert L.lib.votenet_eval_loss_decode(ctypes.byref(b), stream) == 1, change
    assert L.lib.votenet_eval_loss(ctypes.byref(a), None, None, stream) == 1
    torch.cuda.synchronize()
    assert torch.equal(stats, stats_before)


@pytest.mark.parametrize("tag", ["scannet", "sunrgbd"])
def test_get_loss_fused_matches_the_tensor_formulation(tag, monkeypatch):
    V, losses, fused = _modules()
    cfg = V.scannet_config() if tag == "scannet" else V.sunrgbd_config()
    _, ep = golden_end_points(tag, DEV)
    monkeypatch.setenv("VOTENET_FUSED_LOSS", "0")
    want_loss, want = V.get_loss(dict(ep), cfg)
    monkeypatch.setenv("VOTENET_FUSED_LOSS", "1")
    calls = []
    real = fused._launch_eval
    monkeypatch.setattr(fused, "_launch_eval", lambda name, *a: (calls.append(name), real(name, *a)))
    got_loss, got = V.get_loss(dict(ep), cfg)
    torch.cuda.synchronize()
    assert calls == ["votenet_eval_loss_decode", "votenet_eval_loss"]  # the dispatch took the kernels
    assert float(got_loss) == float(got["detection_loss"])
    for key in losses.EVAL_STAT_KEYS:
        w, g = float(want[key]), float(got[key])
        print("%s %-20s fused %.9g tensor %.9g" % (tag, key, g, w))
        assert abs(g - w) <= 1e-5 * max(1.0, abs(w)), (key, g, w)
    for key in LABELS:
        assert got[key].dtype == want[key].dtype and torch.equal(got[key], want[key]), key
    assert int(got["objectness_label"].sum()) > 0
    for key in ("iou_labels", "pred_bbox"):
        assert got[key].shape == want[key].shape
        np.testing.assert_allclose(got[key].cpu().numpy(), want[key].cpu().numpy(), rtol=0, atol=1e-6, err_msg=key)


# ------------------------------------------------------------------ end to end
def _detector_and_batches():
    from test_inference_gpu import _detector, _mods
    U, V, I, step, data = _mods()
    det, cfg = _detector(V, step, "scannet")
    config_dict = {"dataset_config": cfg, "remove_empty_box": False, "use_3d_nms": True, "nms_iou": 0.25,
                   "use_old_type_nms": False, "cls_nms": True, "use_iou_for_nms": False,
                   "per_class_proposal": True, "conf_thresh": 0.05}
    batches = [data.make_batch(b, 20000, cfg, seed=40 + s, device=DEV) for s, b in enumerate((4, 2))]
    return V, I, det, cfg, config_dict, batches


def _same_metrics(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert set(g) == set(w)
        for key, val in w.items():
            assert g[key] == val or (math.isnan(val) and math.isnan(g[key])), (key, g[key], val)


def test_evaluate_with_loss_end_to_end():
    V, I, det, cfg, config_dict, batches = _detector_and_batches()
    losses = importlib.import_module("3dioumatch_amd.votenet.losses")
    O = importlib.import_module("3dioumatch_amd.votenet.iou_opt")
    engine = I.InferenceEngine(det)
    plain = I.evaluate(engine, batches, config_dict, device_ap=True)
    metrics, stats = I.evaluate(engine, batches, config_dict, device_ap=True, with_loss=True)
    _same_metrics(metrics, plain)
    assert set(stats) == set(losses.EVAL_STAT_KEYS) | {"mean_loss"} and stats["mean_loss"] == stats["detection_loss"]
    per_batch = []
    for batch in batches:
        with torch.no_grad():
            ep = det({"point_clouds": batch["point_clouds"]})
        ep.update({k: v for k, v in batch.items() if k not in ep})
        per_batch.append({k: float(v) for k, v in V.get_loss(ep, cfg)[1].items() if k in losses.EVAL_STAT_KEYS})
    for key in losses.EVAL_STAT_KEYS:
        want = sum(b[key] for b in per_batch) / len(per_batch)
        print("%-20s evaluate %.9g mean of per-batch get_loss %.9g" % (key, stats[key], want))
    for key in losses.EVAL_STAT_KEYS:
        want = sum(b[key] for b in per_batch) / len(per_batch)
        assert abs(stats[key] - want) <= 1e-4 * max(1.0, abs(want)), (key, stats[key], want)
    # the plain loop gives the same, and the optimised boxes are what the loss reads
    metrics0, stats0 = O.evaluate(det, batches, config_dict, opt_step=0, device_ap=True, with_loss=True)
    _same_metrics(metrics0, O.evaluate(det, batches, config_dict, opt_step=0, device_ap=True))
    for key in losses.EVAL_STAT_KEYS:
        assert abs(stats0[key] - stats[key]) <= 1e-4 * max(1.0, abs(stats[key])), (key, stats0[key], stats[key])
    _, stats2 = O.evaluate(det, batches, config_dict, opt_step=2, opt_rate=1e-2, device_ap=True, with_loss=True)
    print("center_loss opt_step=0 %.9g opt_step=2 %.9g" % (stats0["center_loss"], stats2["center_loss"]))
    assert stats2["center_loss"] != stats0["center_loss"]


def test_evaluate_names_the_missing_label():
    V, I, det, cfg, config_dict, batches = _detector_and_batches()
    short = [{k: v for k, v in batches[1].items() if k != "vote_label_mask"}]
    with pytest.raises(ValueError, match="vote_label_mask"):
        I.evaluate(I.InferenceEngine(det), short, config_dict, device_ap=True, with_loss=True)
