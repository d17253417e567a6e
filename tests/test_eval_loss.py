"""The test-time criterion (votenet/losses.py:get_loss, the mirror of models/loss_helper.py:222-291), its
fused form's arithmetic on the host, the epoch meter and the public switches -- without a GPU.

  * losses.get_loss (tensor formulation) against the REFERENCE's own get_loss on seeded inputs
    (tests/golden/eval_loss_ref.npz, made by tests/golden/make_eval_loss_golden.py): the 20 logged statistics
    within 2e-5 * max(1, |ref|) (the bound of tests/test_fused_loss.py::_compare against its goldens), the
    objectness labels / mask / assignment equal -- proposals next to the origin are assigned the FIRST empty
    slot --, iou_labels within 1e-7 and pred_bbox within 1e-6 as tests/test_train_step.py holds
    compute_iou_labels to.
  * the same tensor formulation on the planted cases of tests/eval_loss_cases.py against their float64 truth (labels
    equal, statistics to the same 2e-5): the plants and the first-index rule hold for the formulation the GPU tests
    compare the kernels with.
  * the eval functions of csrc/loss_core.h compiled with g++ (tests/eval_loss_host.cpp) and driven through the
    binding's pass builder (fused_loss._eval_pass) against the float64 truth of tests/eval_loss_cases.py on every
    shape of loss_kernel_cases.CASES and a case without a positive: statistics within
    1e-5 * max(1, |ref|) (tests/test_loss_kernels.py derives the bound), labels equal, the decoded boxes within one
    rounding per operation.
  * the planted proposals make the criterion's numbers differ from the training criterion's on the same inputs
    by more than 1e-3 (the schedule-error scale of tests/test_loss_kernels.py): an alias to the training kernels
    cannot pass.
  * EvalLossMeter on the tensor path: three batches of 3, 2 and 1 scenes give the plain mean of the per-batch
    values; an empty meter raises; a batch without a label key raises a ValueError that names it.
  * both evaluate functions have with_loss=False.
"""
import ctypes
import importlib
import inspect
import os
import subprocess

import numpy as np
import pytest
import torch

import eval_loss_cases as cases
import loss_kernel_cases as base
from conftest import golden, load_pkg
from loss_kernel_cases import CASES

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-5
LABELS = ("objectness_label", "objectness_mask", "object_assignment")
SRC_KEYS = ("center_label", "box_label_mask", "heading_class_label", "heading_residual_label", "size_class_label",
            "size_residual_label", "sem_cls_label", "vote_label", "vote_label_mask", "seed_inds", "seed_xyz")
HEAD_KEYS = ("obj", "center", "h_scores", "h_resn", "s_scores", "s_resn", "sem", "iou", None, "vote_xyz")


@pytest.fixture(scope="module")
def eval_host_build():
    so = os.path.join(HERE, "_eval_loss_host.so")
    src = os.path.join(HERE, "eval_loss_host.cpp")
    core = os.path.join(os.path.dirname(HERE), "3dioumatch_amd", "csrc", "loss_core.h")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(core)):
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-o", so, src])
    return ctypes.CDLL(so)


def _modules():
    load_pkg()
    return (importlib.import_module("3dioumatch_amd.votenet"),
            importlib.import_module("3dioumatch_amd.votenet.losses"),
            importlib.import_module("3dioumatch_amd.votenet.fused_loss"))


class _Config:
    """the one thing the binding asks of a dataset config"""

    def __init__(self, mean_size):
        self._mean_size = mean_size

    def mean_size(self, dev):
        return self._mean_size.to(dev)


# ------------------------------------------------------------------ the pass builder on a case (both legs)
def run_case(fused, dev, c, monkeypatch, accum=None):
    """fused_loss._eval_pass on the tensors of a case, the IoU kernel replaced by the case's planted IoU labels
    -> dict of numpy outputs (stats, labels, iou_labels, pred_bbox, and the boxes handed to the IoU kernel)"""
    t = base.tensors(c, dev)
    size_residuals = t["size_residuals"]
    if c["layout"] == "strided":
        size_residuals = base.strided4(size_residuals)
    seen = {}

    def scene_iou(boxes, gt_boxes):
        seen["boxes"], seen["gt_boxes"] = boxes.clone(), gt_boxes.clone()
        return t["iou_lab"], t["iou_assign"]

    src = {k: t[k] for k in SRC_KEYS}
    src["aggregated_vote_xyz"] = t["agg_xyz"]
    heads = [None if k is None else t[k] for k in HEAD_KEYS]
    with monkeypatch.context() as mp:
        mp.setattr(fused, "_scene_iou", scene_iou)
        stats, lab, mask, assign, iou_labels, pred_bbox = fused._eval_pass(
            src, _Config(t["mean_size"]), heads, size_residuals, accum)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert torch.equal(pred_bbox, seen["boxes"]) and iou_labels is t["iou_lab"]
    return dict(stats=stats.cpu().numpy(), objectness_label=lab.cpu().numpy(), objectness_mask=mask.cpu().numpy(),
                object_assignment=assign.cpu().numpy(), boxes=seen["boxes"].cpu().numpy(),
                gt_boxes=seen["gt_boxes"].cpu().numpy())


def check_case(c, ref, out, what, tol=TOL):
    """labels equal, boxes within their rounding-count bounds, every statistic within tol * max(1, |ref|);
    prints each figure first; returns the worst statistic error"""
    for name in ("objectness_label", "object_assignment"):
        assert out[name].dtype == np.int64 and np.array_equal(out[name], ref[name]), (what, name)
    assert np.array_equal(out["objectness_mask"].astype(np.float64), ref["objectness_mask"]), what
    for name in ("boxes", "gt_boxes"):
        err = np.abs(out[name].astype(np.float64) - ref[name])
        assert np.isfinite(out[name]).all() and (err <= ref[name + "_bound"]).all(), (what, name, err.max())
    assert (out["boxes"][:, :, 3:6][ref["clamped"]] == np.float32(1e-6)).all()
    worst = {}
    for i, name in enumerate(cases.STAT_KEYS):
        want, got = ref["stats"][name], float(out["stats"][i])
        worst[name] = abs(got - want) / max(1.0, abs(want))
        print("%s stat %-20s got %.9g want %.9g err %.3g" % (what, name, got, want, worst[name]))
    print("%s WORST stat %.3g (%s)" % (what, max(worst.values()), max(worst, key=worst.get)))
    for name, err in worst.items():
        assert err <= tol, (what, name, err)
    return max(worst.values())


def check_plants(c, ref):
    """the planted proposals are what they claim to be, by the float64 truth of both criteria"""
    p = c["planted"]
    if p is None:
        return
    ps = p["scene"]
    train = base.reference(c["name"])
    lab, assign = ref["objectness_label"], ref["object_assignment"]
    # (a) positive here, negative for the training criterion, assigned the first of the tied empty slots
    assert lab[ps, p["ka"]] == 1 and train["objectness_label"][ps, p["ka"]] == 0
    assert assign[ps, p["ka"]] == p["first_empty"] and c["box_label_mask"][ps, p["first_empty"]] != 1
    assert (c["box_label_mask"][ps] != 1).sum() >= 2  # (a real tie)
    pred = np.argmax(c["sem"], -1)[ps]
    cls = c["sem_cls_label"][ps]
    # (b) a positive whose predicted class is neither its assigned box's nor its best-IoU box's
    assert lab[ps, p["kb"]] == 1 and pred[p["kb"]] != cls[assign[ps, p["kb"]]]
    assert pred[p["kb"]] != cls[c["iou_assign"][ps, p["kb"]]]
    # (c) a negative with a matching class
    assert lab[ps, p["kc"]] == 0 and pred[p["kc"]] == cls[assign[ps, p["kc"]]]
    assert ref["stats"]["cls_acc"] != ref["stats"]["cls_acc_obj"]
    if c["B"] > 1:  # the all-empty scene: every proposal negative, assigned slot 0
        assert not lab[0].any() and (assign[0] == 0).all()


def _host_case(name, no_positive, eval_host_build, monkeypatch):
    _, _, fused = _modules()
    monkeypatch.setattr(fused, "_EVAL_HOST_BUILD", eval_host_build)
    c, ref = cases.build(name, no_positive), cases.reference(name, no_positive)
    check_plants(c, ref)
    out = run_case(fused, torch.device("cpu"), c, monkeypatch)
    return c, ref, out


# ------------------------------------------------------------------ end_points of a case
def case_config(V, c):
    return V.DatasetConfig(c["NC"], c["NH"], c["NS"], mean_size_arr=c["mean_size"])


def case_end_points(c, dev):
    """the case as the end_points of an eval forward plus its labels (head outputs in the case's layout)"""
    t = base.tensors(c, dev)
    ep = {k: t[k] for k in SRC_KEYS}
    ep.update(aggregated_vote_xyz=t["agg_xyz"], objectness_scores=t["obj"], center=t["center"],
              heading_scores=t["h_scores"], heading_residuals_normalized=t["h_resn"],
              heading_residuals=t["h_resn"] * (np.pi / c["NH"]), size_scores=t["s_scores"],
              size_residuals_normalized=t["s_resn"], size_residuals=t["size_residuals"],
              sem_cls_scores=t["sem"], iou_scores=t["iou"], vote_xyz=t["vote_xyz"])
    return ep, t


def tensor_case(V, losses, fused, c, dev, monkeypatch):
    """losses.get_loss' tensor formulation (fused path off) on a case with the planted IoU labels -> the
    numpy outputs check_case reads (no boxes: the tensor formulation decodes them itself)"""
    ep, t = case_end_points(c, dev)
    with monkeypatch.context() as mp:
        mp.setenv("VOTENET_FUSED_LOSS", "0")
        mp.setattr(losses, "_scene_best_iou", lambda boxes, gt: (t["iou_lab"], t["iou_assign"].long()))
        _, ep = V.get_loss(ep, case_config(V, c))
    stats = [float(ep[k]) for k in losses.EVAL_STAT_KEYS] + [float(ep["objectness_label"].sum())]
    return dict(stats=np.array(stats, np.float64), objectness_label=ep["objectness_label"].cpu().numpy(),
                objectness_mask=ep["objectness_mask"].cpu().numpy(),
                object_assignment=ep["object_assignment"].cpu().numpy(), pred_bbox=ep["pred_bbox"].cpu().numpy())


def stat_errors(ref, out):
    return {name: abs(float(out["stats"][i]) - ref["stats"][name]) / max(1.0, abs(ref["stats"][name]))
            for i, name in enumerate(cases.STAT_KEYS)}


@pytest.mark.parametrize("name", list(CASES))
def test_tensor_formulation_on_the_cases(name, monkeypatch):
    """losses.get_loss in fp32 on the planted cases against the float64 truth: labels equal (the first-index
    rule between identical empty slots included), statistics within 2e-5 * max(1, |ref|), the bound it is held
    to against the reference's golden"""
    V, losses, fused = _modules()
    c, ref = cases.build(name), cases.reference(name)
    out = tensor_case(V, losses, fused, c, torch.device("cpu"), monkeypatch)
    for key in LABELS:
        assert np.array_equal(out[key].astype(np.float64), ref[key].astype(np.float64)), key
    err = stat_errors(ref, out)
    print("%s tensor formulation WORST %.3g (%s)" % (name, max(err.values()), max(err, key=err.get)))
    assert max(err.values()) <= 2e-5, err
    np.testing.assert_allclose(out["pred_bbox"], ref["boxes"], rtol=0, atol=1e-5)


# ------------------------------------------------------------------ tensor formulation against the reference
def golden_end_points(tag, dev, scenes=None):
    g = golden("eval_loss_ref.npz")
    prefix = tag + "_in::"
    ep = {k[len(prefix):]: torch.from_numpy(g[k]).to(dev) for k in g.files if k.startswith(prefix)}
    if scenes is not None:
        ep = {k: v[list(scenes)].contiguous() for k, v in ep.items()}
    return g, ep


def _oracle_iou(losses, oracle, monkeypatch):
    monkeypatch.setattr(losses, "boxes_iou3d_gpu", lambda a, b: torch.from_numpy(
        oracle.boxes_iou3d(a.detach().numpy(), b.detach().numpy())))


@pytest.mark.parametrize("tag", ["scannet", "sunrgbd"])
def test_get_loss_matches_reference_golden(tag, oracle_omp, monkeypatch):
    V, losses, _ = _modules()
    _oracle_iou(losses, oracle_omp, monkeypatch)
    cfg = V.scannet_config() if tag == "scannet" else V.sunrgbd_config()
    g, ep = golden_end_points(tag, torch.device("cpu"))
    inputs = {k: v.clone() for k, v in ep.items()}
    loss, ep = V.get_loss(ep, cfg)
    for k, v in inputs.items():
        assert torch.equal(v, ep[k]), "get_loss changed its input %s" % k
    assert float(loss) == float(ep["detection_loss"]) == float(ep["loss"])
    for key in losses.EVAL_STAT_KEYS:
        want, got = float(g["%s_stat::%s" % (tag, key)]), float(ep[key])
        print("%s %-20s got %.9g want %.9g" % (tag, key, got, want))
        assert abs(got - want) <= 2e-5 * max(1.0, abs(want)), (key, got, want)
    for key in LABELS:
        want = g["%s_%s" % (tag, key)]
        assert np.array_equal(ep[key].numpy().astype(np.float64), want.astype(np.float64)), key
    assert ep["objectness_label"].dtype == torch.int64 and ep["object_assignment"].dtype == torch.int64
    # the first-index rule: the proposals next to the origin take the first of the three identical empty slots
    valid = int(ep["box_label_mask"][0].sum())
    assert (ep["object_assignment"][:, :4] == valid).all() and (ep["objectness_label"][:, :4] == 1).all()
    np.testing.assert_allclose(ep["iou_labels"].numpy(), g[tag + "_iou_labels"], rtol=0, atol=1e-7)
    np.testing.assert_allclose(ep["pred_bbox"].numpy(), g[tag + "_pred_bbox"], rtol=0, atol=1e-6)


# ------------------------------------------------------------------ the host build against float64
@pytest.mark.parametrize("name", list(CASES))
def test_host_build_against_float64(name, eval_host_build, monkeypatch):
    c, ref, out = _host_case(name, False, eval_host_build, monkeypatch)
    check_case(c, ref, out, name)


def test_host_build_no_positive_anywhere(eval_host_build, monkeypatch):
    """no positive proposal and every vote_label_mask zero: every masked term is exactly 0"""
    c, ref, out = _host_case("one_lane_over", True, eval_host_build, monkeypatch)
    check_case(c, ref, out, "one_lane_over no-positive")
    st = dict(zip(cases.STAT_KEYS, out["stats"]))
    for key in ("vote_loss", "heading_cls_loss", "heading_reg_loss", "size_cls_loss", "size_reg_loss", "sem_cls_loss",
                "iou_loss", "cls_acc_obj", "pred_iou_obj_value", "iou_acc_obj", "pos_ratio", "obj_count"):
        assert st[key] == 0.0, key


@pytest.mark.parametrize("name", [n for n in CASES if CASES[n][1] >= 3 and CASES[n][2] >= 2])
def test_planted_keys_differ_from_the_training_criterion(name, eval_host_build, monkeypatch):
    """on the same inputs the training criterion (float64, loss_kernel_cases.reference) gives other numbers for
    the planted keys: by more than 1e-3, so no implementation that routes to the training path passes
    test_host_build_against_float64 / the GPU leg"""
    c, ref, out = _host_case(name, False, eval_host_build, monkeypatch)
    train = base.reference(name)["stats"]
    got = dict(zip(cases.STAT_KEYS, out["stats"]))
    keys = cases.PLANTED_KEYS + (cases.PLANTED_KEYS_CLASS_IOU if c["NI"] > 1 else ())
    for key in keys:
        print("%s %-12s eval %.6g training %.6g" % (name, key, got[key], train[key]))
        assert abs(got[key] - train[key]) > 1e-3, (name, key)
        assert abs(got[key] - ref["stats"][key]) <= TOL * max(1.0, abs(ref["stats"][key])), (name, key)
    p = c["planted"]
    assert out["objectness_label"][p["scene"], p["ka"]] == 1
    assert base.reference(name)["objectness_label"][p["scene"], p["ka"]] == 0


# ------------------------------------------------------------------ the epoch meter, tensor path
def test_meter_is_the_plain_mean_of_per_batch_values(oracle_omp, monkeypatch):
    V, losses, _ = _modules()
    _oracle_iou(losses, oracle_omp, monkeypatch)
    cfg, dev = V.scannet_config(), torch.device("cpu")
    meter = V.EvalLossMeter(dev)
    per_batch = []
    for scenes in ((0, 1, 0), (1, 0), (1,)):
        _, ep = golden_end_points("scannet", dev, scenes)
        loss, ep = meter.step(ep, cfg)
        assert float(loss) == float(ep["detection_loss"])
        _, again = golden_end_points("scannet", dev, scenes)
        per_batch.append({k: float(v) for k, v in V.get_loss(again, cfg)[1].items() if k in losses.EVAL_STAT_KEYS})
    assert meter.batches == 3
    assert per_batch[0]["detection_loss"] != per_batch[2]["detection_loss"]
    result = meter.result()
    assert set(result) == set(losses.EVAL_STAT_KEYS) | {"mean_loss"}
    for key in losses.EVAL_STAT_KEYS:
        want = sum(b[key] for b in per_batch) / 3
        assert abs(result[key] - want) <= 1e-6 * max(1.0, abs(want)), (key, result[key], want)
    assert result["mean_loss"] == result["detection_loss"]


def test_meter_without_batches_and_batches_without_labels_raise(monkeypatch):
    V, losses, _ = _modules()
    with pytest.raises(ValueError, match="no batch"):
        V.EvalLossMeter(torch.device("cpu")).result()
    _, ep = golden_end_points("scannet", torch.device("cpu"))
    for key in ("vote_label", "sem_cls_label"):
        short = {k: v for k, v in ep.items() if k != key}
        with pytest.raises(ValueError, match=key):
            V.EvalLossMeter(torch.device("cpu")).step(short, V.scannet_config())
        with pytest.raises(ValueError, match=key):
            V.get_loss(short, V.scannet_config())


def test_evaluate_functions_have_with_loss_off_by_default():
    load_pkg()
    for module in ("inference", "iou_opt"):
        fn = importlib.import_module("3dioumatch_amd.votenet." + module).evaluate
        assert inspect.signature(fn).parameters["with_loss"].default is False, module
