"""Device-resident AP evaluation on the MI355X: the match kernel (csrc/eval_ap.hip) against the
oracle stand-in, the reference's golden AP with both kernels, parity of DeviceAPCalculator with the
host path (APCalculator / eval_det) on end points with shifted and duplicated true boxes, the absence
of host synchronisation in the per-batch calls, and evaluate(..., device_ap=True) of both evaluation
loops against device_ap=False."""
import importlib

import numpy as np
import pytest
import torch

from conftest import golden, load_pkg
from test_eval_det import _perfect_end_points, _random_corners
from test_eval_device import check_golden_ap, standin_match

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CLASSES = (0, 1, 2, 4)      # of C = 5: class 3 has no ground truth


def _mods():
    load_pkg()
    return (importlib.import_module("3dioumatch_amd.votenet"),
            importlib.import_module("3dioumatch_amd.votenet.eval_det"),
            importlib.import_module("3dioumatch_amd.votenet.eval_helper"))


def _match_case(rng, b=3, k=40, g=70, bases=17):
    """Boxes of _random_corners(spread 1.5).  Independent random boxes would leave about 55 of the 600
    slots above IoU 0.25 (measured with the oracle), so a scene is built from `bases` random boxes:
    ground-truth slot j < 4 * bases is base box j % bases moved by 3 cm per copy along x, its four
    copies in the four classes; proposal i is base box i % bases moved by 1 cm + 2 mm * i along z.
    Every kept proposal then has a box above 0.25 in each class present, and the columns of a class
    lie on both sides of the 64-column tile.  Slot 68 repeats slot 3 with its class (the first index
    must win, across the tile boundary), slot 69 is a free box; about 5 % of the slots are invalid,
    the last scene has no valid slot, a quarter of the proposals is not kept."""
    det = np.zeros((b, k, 8, 3), np.float32)
    gt = np.zeros((b, g, 8, 3), np.float32)
    gt_cls = np.zeros((b, g), np.int64)
    for s in range(b):
        base = _random_corners(rng, bases, 1.5)
        for i in range(k):
            det[s, i] = base[i % bases] + np.array([0, 0, 0.01 + 0.002 * i], np.float32)
        for j in range(4 * bases):
            gt[s, j] = base[j % bases] + np.array([0.03 * (j // bases), 0, 0], np.float32)
            gt_cls[s, j] = CLASSES[(j // bases + j % bases) % 4]
        gt[s, 4 * bases:] = _random_corners(rng, g - 4 * bases, 1.5)
        gt_cls[s, 4 * bases:] = rng.choice(CLASSES, g - 4 * bases)
        gt[s, 68], gt_cls[s, 68] = gt[s, 3], gt_cls[s, 3]
    keep = rng.random((b, k)) > 0.25
    valid = rng.random((b, g)) > 0.05
    valid[:, [3, 68]] = True
    valid[b - 1] = False
    det_cls = rng.choice(CLASSES + (3,), (b, k))
    keep[:, 3], det_cls[:, 3] = True, gt_cls[:, 3]      # proposal 3 competes for the repeated box
    return det, keep, det_cls, gt, valid, gt_cls


@pytest.mark.parametrize("num_class,enough", [(5, 200), (0, 40)])
def test_match_kernel_matches_oracle(num_class, enough, oracle):
    """B = 3, K = 40, G = 70 (two tiles of ground-truth columns).  `enough`: slots above IoU 0.25 --
    200 of the 600 (proposal, class) slots; in single-class mode there are 120 slots in all, so the
    same third of them."""
    _, D, _ = _mods()
    arrays = _match_case(np.random.default_rng(11))
    dev = [torch.from_numpy(a).to(DEV) for a in arrays]
    ov, jm = D.eval_match_gpu(*dev, num_class)
    wov, wjm = standin_match(oracle)(*[torch.from_numpy(a) for a in arrays], num_class)
    ov, jm, wov, wjm = ov.cpu().numpy(), jm.cpu().numpy(), wov.numpy(), wjm.numpy()
    keep = arrays[1]
    assert ov.shape == wov.shape == (3, 40, max(num_class, 1)) and jm.dtype == np.int32
    assert (wov > 0.25).sum() >= enough, (wov > 0.25).sum()
    np.testing.assert_array_equal(jm, wjm)
    assert np.array_equal(np.isneginf(ov), np.isneginf(wov)) and not np.isnan(ov).any()
    fin = np.isfinite(wov)
    np.testing.assert_allclose(ov[fin], wov[fin], rtol=0, atol=1e-13)
    assert np.isneginf(ov[~keep]).all() and (jm[~keep] == -1).all()              # not kept
    assert np.isneginf(ov[2]).all() and (jm[2] == -1).all()                      # no valid ground truth
    assert (jm >= 64).any() and ((jm >= 0) & (jm < 64)).any()                    # both tiles win somewhere
    assert (jm[:2] == 3).any() and not (jm == 68).any()                          # the first of two equal boxes
    if num_class:
        assert np.isneginf(ov[:, :, 3]).all() and (jm[:, :, 3] == -1).all()      # the absent class
        assert (jm[:2][keep[:2]][:, list(CLASSES)] >= 0).all()
    else:
        absent = arrays[2] == 3
        assert absent[keep].any() and (jm[absent] == -1).all()


@pytest.mark.parametrize("num_class", [5, 0])
def test_match_kernel_without_ground_truth_or_detections(num_class):
    _, D, _ = _mods()
    det, keep, det_cls, gt, valid, gt_cls = (torch.from_numpy(a).to(DEV) for a in _match_case(np.random.default_rng(12)))
    ov, jm = D.eval_match_gpu(det, keep, det_cls, gt[:, :0].contiguous(), valid[:, :0].contiguous(),
                              gt_cls[:, :0].contiguous(), num_class)                      # G = 0
    assert tuple(ov.shape) == (3, 40, max(num_class, 1))
    assert torch.isneginf(ov).all() and (jm == -1).all()
    ov, jm = D.eval_match_gpu(det, torch.zeros_like(keep), det_cls, gt, valid, gt_cls, num_class)   # nothing kept
    assert torch.isneginf(ov).all() and (jm == -1).all()
    with pytest.raises(RuntimeError, match="iou3d_eval_match"):                           # K = 0: outside the gate
        D.eval_match_gpu(det[:, :0].contiguous(), keep[:, :0].contiguous(), det_cls[:, :0].contiguous(),
                         gt, valid, gt_cls, num_class)


def test_device_ap_calculator_matches_reference_gpu():
    _, _, E = _mods()
    check_golden_ap(E, DEV)


def _imperfect_end_points(V, cfg, rng):
    """test_eval_det._perfect_end_points with every second true box moved by 0.3 x its size and every
    true box repeated (4 mm off, so that the NMS at 0.999 keeps both) with the same logits."""
    ep = _perfect_end_points(V, cfg, rng, scenes=3, k=48)
    mean = torch.from_numpy(cfg.mean_size_arr.astype(np.float32))
    for b in range(3):
        n = int(ep["box_label_mask"][b].sum())
        assert 0 < n and 2 * n <= 48
        for j in range(1, n, 2):
            size = mean[ep["size_class_label"][b, j]] + ep["size_residual_label"][b, j]
            ep["center"][b, j] += 0.3 * size
        for key in ("center", "objectness_scores", "heading_scores", "heading_residuals", "size_scores",
                    "size_residuals", "sem_cls_scores"):
            ep[key][b, n:2 * n] = ep[key][b, :n]
        ep["center"][b, n:2 * n] += 0.004
    return ep


@pytest.mark.parametrize("per_class", [True, False], ids=["per-class", "single-class"])
@pytest.mark.parametrize("tag", ["scannet", "sunrgbd"])
def test_device_ap_matches_host_path(tag, per_class):
    V, _, E = _mods()
    cfg = V.sunrgbd_config() if tag == "sunrgbd" else V.scannet_config()
    ep = {k: (v.to(DEV) if torch.is_tensor(v) else v)
          for k, v in _imperfect_end_points(V, cfg, np.random.default_rng(3)).items()}
    config_dict = {"dataset_config": cfg, "remove_empty_box": False, "use_3d_nms": True,
                   "nms_iou": 0.999, "use_old_type_nms": False, "cls_nms": True,
                   "use_iou_for_nms": False, "per_class_proposal": per_class, "conf_thresh": 0.05}
    dev = E.DeviceAPCalculator((0.25, 0.5), None)
    dev.step(E.parse_predictions_device(ep, config_dict), E.parse_groundtruths_device(ep, config_dict))
    preds, gts = E.parse_predictions(ep, config_dict), E.parse_groundtruths(ep, config_dict)
    got = dev.compute_metrics()
    partial = tied = False
    for thr, g in zip((0.25, 0.5), got):
        host = E.APCalculator(thr, None, device="cuda:0")
        host.step(preds, gts)
        with np.errstate(invalid="ignore", divide="ignore"):
            want = host.compute_metrics()
        assert list(g) == list(want)
        np.testing.assert_allclose([g[k] for k in want], [want[k] for k in want], rtol=0, atol=1e-12,
                                   equal_nan=True)
        partial |= any(0 < v < 1 for k, v in want.items() if k.endswith("Average Precision"))
    for c in range(cfg.num_class):
        scores = [s for scan in preds for cc, _, s in scan if cc == c]
        tied |= len(set(scores)) < len(scores)
    assert partial and tied      # ordering and first-claim were exercised


def test_per_batch_calls_do_not_synchronise():
    V, _, E = _mods()
    cfg = V.scannet_config()
    config_dict = {"dataset_config": cfg, "remove_empty_box": True, "use_3d_nms": True,
                   "nms_iou": 0.25, "use_old_type_nms": False, "cls_nms": True,
                   "use_iou_for_nms": True, "per_class_proposal": True, "conf_thresh": 0.05}
    ep = {k: (v.to(DEV) if torch.is_tensor(v) else v)
          for k, v in _perfect_end_points(V, cfg, np.random.default_rng(5)).items()}
    calc = E.DeviceAPCalculator()
    calc.step(E.parse_predictions_device(ep, config_dict), E.parse_groundtruths_device(ep, config_dict))  # warm-up
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            ep["center"].cpu()
        except RuntimeError:
            pass
        else:
            pytest.skip("torch.cuda.set_sync_debug_mode('error') does not flag a .cpu() on this build")
        for per_class in (True, False):
            cd = dict(config_dict, per_class_proposal=per_class)
            calc.step(E.parse_predictions_device(ep, cd), E.parse_groundtruths_device(ep, cd))
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    assert calc.scan_cnt == 9 and len(calc.compute_metrics()) == 2


def test_evaluate_device_ap_matches_host_ap():
    V, _, E = _mods()
    I = importlib.import_module("3dioumatch_amd.votenet.inference")
    O = importlib.import_module("3dioumatch_amd.votenet.iou_opt")
    step = importlib.import_module("3dioumatch_amd.votenet.step")
    data = importlib.import_module("3dioumatch_amd.votenet.data")
    cfg = V.scannet_config()
    det = step.build_detector(cfg, seed=0).to(DEV).eval()
    config_dict = {"dataset_config": cfg, "remove_empty_box": False, "use_3d_nms": True, "nms_iou": 0.25,
                   "use_old_type_nms": False, "cls_nms": True, "use_iou_for_nms": False,
                   "per_class_proposal": True, "conf_thresh": 0.05}
    batches = [data.make_batch(4, 20000, cfg, seed=40 + s, device=DEV) for s in range(2)]
    # the second batch's labels arrive on the host
    batches[1] = {k: (v.cpu() if torch.is_tensor(v) and k != "point_clouds" else v) for k, v in batches[1].items()}
    engine = I.InferenceEngine(det)
    for fn, first in ((I.evaluate, engine), (O.evaluate, det)):
        with np.errstate(invalid="ignore", divide="ignore"):
            want = fn(first, batches, config_dict, opt_step=0, device_ap=False)
            got = fn(first, batches, config_dict, opt_step=0, device_ap=True)
        assert len(got) == len(want) == 2
        for g, w in zip(got, want):
            assert list(g) == list(w)
            np.testing.assert_allclose([g[k] for k in w], [w[k] for k in w], rtol=0, atol=1e-12, equal_nan=True)
        assert any(k.endswith("Average Precision") for k in want[0])
