"""The fused loss kernels (csrc/votenet_loss.hip: loss_decode_kernel, loss_terms_kernel,
loss_finalize_kernel; csrc/loss_core.h; votenet/fused_loss.py) against their formulas, directly and at
multi-workgroup shapes.

tests/test_fused_loss.py and the train-step tests reach these kernels through a whole detector at B = 2,
K = 64 and compare parameter gradients fp32 against fp32.  Here the real binding (_loss_pass, the one pass
builder, in both of its modes) is driven without a network on seeded inputs (tests/loss_kernel_cases.py) and
every output is compared with a float64 evaluation of the formulas:

  * objectness_label / objectness_mask / object_assignment / gt_nearest: equal;
  * the decoded boxes handed to the IoU kernel: within one fp32 rounding per operation;
  * every statistic within 1e-5 * max(1, |ref|); every gradient element within 1e-5 * max|ref of its
    tensor|; elements whose reference is exactly 0 (rows of non-positive proposals, g_obj in consistency
    mode, votes of masked seeds) exactly 0;
  * guard words: the gradients go through `grad_dest` into one sentinel-filled buffer, and the launches are
    repeated through the entry points with the same VnLossArgs but every output (boxes, statistics, labels,
    gt_nearest, the partial rows, the gradients) inside sentinel-filled buffers of the test's own: 64 guard
    words on both sides untouched, no sentinel left inside, and bit-equal to what the binding returned.

The shapes are loss_kernel_cases.CASES: one to eight proposal workgroups per scene, the GT workgroup's
stride loop at G = 256, 25 and more partial rows, rows wider than kRowMax.  The float32 evaluation of the
same reference lies within 5e-7 of float64 on these inputs; a schedule error (a dropped lane, block or
partial row, a double count) moves a statistic by 1e-3 or more and a gradient row by order 1, so the bound
of 1e-5 is 20x the former and 100x under the latter.

CPU leg: the same cases through the host build of loss_core.h (tests/loss_host.cpp): proves the builder,
its margins and the reference without a GPU.  GPU leg: the kernels.

The gradient sizes and shapes of the arenas come from the binding's one table (_grad_layout); the float64
reference's own shapes are asserted against them.  The semi-supervised node (both modes of the pass builder on
one zero-filled gradient buffer) is compared with the two separate nodes on two of the shapes, on both legs:
every output the same bits, every gradient element the same number.

Largest errors seen on the MI355X against float64 (statistic: |err| / max(1, |ref|); gradient: |err| /
max|ref|), over the supervised and consistency runs of each case:
  per case (statistic / gradient): workload_block 3.2e-8 / 3.2e-7, consistency 7.9e-8 / 2.9e-7;
  second_block 1.5e-7 / 3.8e-7, consistency 6.4e-8 / 3.3e-7; one_lane_over 6.6e-8 / 4.5e-7, consistency
  1.3e-7 / 4.1e-7; limits_wide_rows 9.7e-8 / 5.4e-7, consistency 6.5e-8 / 2.2e-7; k_limit 1.9e-7 / 3.9e-7;
  smallest 6.2e-8 / 2.0e-7; no positive 2.2e-8 / 4.5e-7, consistency 7.5e-8 / 2.1e-7.
  per statistic: box_loss 8.3e-8, center_loss 3.3e-8, cls_acc 4.6e-8, heading_cls_loss 6.5e-8,
  heading_reg_loss 5.8e-8, iou_acc 2.2e-8, iou_acc_obj 4.7e-8, iou_loss 1.4e-8, jitter_iou_acc 2.2e-8,
  jitter_iou_acc_obj 2.2e-8, jitter_iou_loss 7.5e-9, loss 1.5e-7, neg_ratio 4.0e-8, obj_acc 4.6e-8,
  obj_count 0, objectness_loss 4.5e-8, pos_ratio 1.2e-8, pred_iou_obj_value 4.6e-8, pred_iou_value 7.1e-8,
  sem_cls_loss 9.7e-8, size_cls_loss 1.3e-7, size_reg_loss 6.2e-8, vote_loss 1.9e-7.
  per tensor: g_center 2.1e-7, g_h_resn 2.0e-7, g_h_scores 5.4e-7, g_iou 3.9e-7, g_iou_jit 4.5e-7, g_obj 2.9e-7,
  g_s_resn 1.3e-7, g_s_scores 3.9e-7, g_sem 4.0e-7, g_vote 4.6e-8.
  Labels, masks, assignments and gt_nearest equal everywhere; boxes at most 0.99 of their rounding-count bound.
The bound stays at 1e-5.
"""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from conftest import load_pkg
from loss_kernel_cases import CASES, CONSISTENCY_CASES, GRAD_OF, SCALED, build, reference, tensors
from test_fused_loss import host_build  # noqa: F401  (fixture: tests/loss_host.cpp compiled with g++)

TOL = 1e-5
GUARD = 64
SENTINEL = {torch.float32: -12345.678, torch.int32: -7777777, torch.int64: -7777777777}
INVALID = 1  # hipErrorInvalidValue


class Arena:
    """named output buffers inside ONE sentinel-filled tensor, GUARD words before, between and behind"""

    def __init__(self, dev, dtype, sizes):
        self.slots, at = {}, GUARD
        for name, n in sizes.items():
            self.slots[name] = (at, int(n))
            at += int(n) + GUARD
        self.buf = torch.full((at,), SENTINEL[dtype], dtype=dtype, device=dev)

    def ptr(self, name):
        return self.buf.data_ptr() + self.slots[name][0] * self.buf.element_size()

    def get(self, name, shape=None):
        at, n = self.slots[name]
        out = self.buf[at:at + n].cpu().numpy()
        return out if shape is None else out.reshape(shape)

    def check(self, what, written=True, untouched=()):
        """guards untouched; written: no sentinel left inside; not written (or named in `untouched`):
        nothing but sentinels"""
        host = self.buf.cpu()
        sent = torch.tensor(SENTINEL[host.dtype], dtype=host.dtype)
        inside = torch.zeros(host.shape, dtype=torch.bool)
        for name, (at, n) in self.slots.items():
            inside[at:at + n] = True
            left = int((host[at:at + n] == sent).sum())
            full = written and name not in untouched
            assert left == (0 if full else n), "%s %s: %d of %d words %s" % (
                what, name, left, n, "never written" if full else "still hold the sentinel")
        assert bool((host[~inside] == sent).all()), "%s: a guard word was overwritten" % what


class _Config:
    """the one thing the binding asks of a dataset config"""

    def __init__(self, mean_size):
        self._mean_size = mean_size

    def mean_size(self, dev):
        return self._mean_size.to(dev)


def _layout(fused, c):
    """the gradients of the case's mode from the binding's one table: name -> (floats per scene, floats, shape)"""
    dims = {"K": c["K"], "NH": c["NH"], "NS": c["NS"], "NC": c["NC"], "NI": c["NI"], "S*VF": c["S"] * c["VF"],
            "jitter": c["jitter"]}
    layout = fused._grad_layout(dims, c["B"])
    return {name: layout[name] for name in (("g_obj",) + fused._CONSISTENCY_GRADS if c["consistency"] else fused._GRADS)}


def _grad_sizes(fused, c):
    return {name: g.size for name, g in _layout(fused, c).items()}


def _grad_shapes(fused, c):
    return {name: g.shape for name, g in _layout(fused, c).items()}


class Run:
    """One pass of the binding over a case.  `out`: what the binding returned (gradients read out of the
    grad_dest arena); `own`: the same launches repeated with every output in the test's arenas; `args`: a
    copy of the VnLossArgs whose outputs point into those arenas (alive as long as this object)."""


def run_case(fused, dev, c, grad_scale, monkeypatch):
    t = tensors(c, dev)
    run = Run()
    run.keep, run.on_gpu = [t], dev.type == "cuda"
    cfg = _Config(t["mean_size"])
    f32, i32, i64 = torch.float32, torch.int32, torch.int64
    B, K, G = c["B"], c["K"], c["G"]
    rows = 2 * K if c["jitter"] else K
    run.grads = Arena(dev, f32, _grad_sizes(fused, c))
    run.own = {}
    seen = {}
    real_launch = fused._launch

    def own_outputs(a):
        """the test's arenas in place of every output of the call"""
        b = type(a).from_buffer_copy(a)
        if "f" not in run.own:
            sizes = dict(stats=fused.ST_COUNT, objectness_mask=B * K, partials=fused._scratch_floats(a, dev))
            sizes.update(_grad_sizes(fused, c))
            run.own.update(f=Arena(dev, f32, sizes), l=Arena(dev, i64, dict(objectness_label=B * K,
                                                                             object_assignment=B * K)),
                           i=Arena(dev, i32, dict(gt_nearest=B * G)),
                           boxes=Arena(dev, f32, dict(boxes=B * rows * 7, gt_boxes=B * G * 7)))
        for arena in run.own.values():
            for name in arena.slots:
                setattr(b, name, arena.ptr(name))
        return b

    def launch(name, a, d):
        real_launch(name, a, d)
        seen.setdefault("calls", []).append(name)
        real_launch(name, own_outputs(a), d)
        if name == "votenet_loss_forward_backward":
            run.args = own_outputs(a)

    def scene_iou(boxes, gt_boxes):
        seen["boxes"], seen["gt_boxes"] = boxes.clone(), gt_boxes.clone()
        return t["iou_lab"], t["iou_assign"]

    monkeypatch.setattr(fused, "_launch", launch)
    monkeypatch.setattr(fused, "_scene_iou", scene_iou)
    dest = {name: run.grads.ptr(name) for name in run.grads.slots}
    heads = [t[k] for k in ("obj", "center", "h_scores", "h_resn", "s_scores", "s_resn", "sem")]
    if c["consistency"]:
        src = {"center": t["center_label"], "mask": t["box_label_mask"],
               "heading_class": t["heading_class_label"], "heading_residual": t["heading_residual_label"],
               "size_class": t["size_class_label"], "size_residual": t["size_residual_label"],
               "sem_cls": t["sem_cls_label"], "aggregated_vote_xyz": t["agg_xyz"]}
        calls = ["votenet_loss_forward_backward"]
    else:
        src = {k: t[k] for k in ("center_label", "box_label_mask", "heading_class_label", "heading_residual_label",
                                 "size_class_label", "size_residual_label", "sem_cls_label", "vote_label",
                                 "vote_label_mask", "seed_inds", "seed_xyz", "jitter_center", "jitter_size",
                                 "jitter_heading")}
        src["aggregated_vote_xyz"] = t["agg_xyz"]
        heads += [t["iou"], t["iou_jit"] if c["jitter"] else None, t["vote_xyz"]]
        calls = ["votenet_loss_decode", "votenet_loss_forward_backward"]
    stats, lab, mask, assign, pred_bbox, _, _ = fused._loss_pass(c["consistency"], src, cfg, heads, grad_dest=dest,
                                                                 grad_scale=grad_scale)
    assert seen["calls"] == calls
    if not c["consistency"]:
        assert torch.equal(pred_bbox, seen["boxes"][:, :K])
    if dev.type == "cuda":
        torch.cuda.synchronize()
    monkeypatch.undo()
    run.out = dict(stats=stats.cpu().numpy(), objectness_label=lab.cpu().numpy(), objectness_mask=mask.cpu().numpy(),
                   object_assignment=assign.cpu().numpy())
    for key in ("boxes", "gt_boxes"):
        if key in seen:
            run.out[key] = seen[key].cpu().numpy()
    shapes = _grad_shapes(fused, c)
    for name in run.grads.slots:
        run.out[name] = run.grads.get(name, shapes[name] if run.grads.slots[name][1] else None)
    return run


def _stat_names(fused, c):
    if c["consistency"]:
        names = {k[len("unlabeled_"):]: i for k, i in fused._CONSISTENCY_KEYS.items()}
    else:
        names = dict(fused._STAT_KEYS)
        if c["jitter"]:
            names.update(fused._JITTER_KEYS)
    names["loss"] = fused.ST_LOSS
    return names


def check_case(fused, c, run, ref, what):
    out, shapes = run.out, _grad_shapes(fused, c)
    # ---- the guard words, and the binding's outputs against the test's own launch of the same arguments
    run.grads.check(what + " grad_dest")
    for key, arena in run.own.items():
        # (the host build sums in one pass: it has no partial rows)
        arena.check(what + " own " + key, written=(key != "boxes" or not c["consistency"]),
                    untouched=() if run.on_gpu else ("partials",))
    own_f, own_l, own_i = run.own["f"], run.own["l"], run.own["i"]
    for name in run.grads.slots:
        assert np.array_equal(own_f.get(name).view(np.int32), out[name].reshape(-1).view(np.int32)), name
    assert np.array_equal(own_f.get("stats").view(np.int32), out["stats"].view(np.int32))
    assert np.array_equal(own_f.get("objectness_mask"), out["objectness_mask"].reshape(-1))
    for name in ("objectness_label", "object_assignment"):
        assert np.array_equal(own_l.get(name), out[name].reshape(-1)), name
    # ---- integer outputs
    for name in ("objectness_label", "object_assignment"):
        assert out[name].dtype == np.int64 and np.array_equal(out[name], ref[name]), (what, name)
    assert np.array_equal(out["objectness_mask"].astype(np.float64), ref["objectness_mask"]), what
    assert np.array_equal(own_i.get("gt_nearest", ref["gt_nearest"].shape), ref["gt_nearest"]), (what, "gt_nearest")
    # ---- the decode launch
    if not c["consistency"]:
        for name in ("boxes", "gt_boxes"):
            assert np.array_equal(run.own["boxes"].get(name).view(np.int32), out[name].reshape(-1).view(np.int32)), name
            err = np.abs(out[name].astype(np.float64) - ref[name])
            print("%s %s: max error %.3g, worst error / bound %.3f" % (
                what, name, err.max(), (err / np.maximum(ref[name + "_bound"], 1e-300))[err > 0].max(initial=0.0)))
            assert np.isfinite(out[name]).all() and (err <= ref[name + "_bound"]).all(), (what, name)
        assert (out["boxes"][:, :c["K"], 3:6][ref["clamped"]] == np.float32(1e-6)).all()
    # ---- statistics
    worst = {}
    for name, i in sorted(_stat_names(fused, c).items()):
        want, got = ref["stats"][name], float(out["stats"][i])
        err = abs(got - want) / max(1.0, abs(want))
        worst[name] = err
        print("%s stat %-20s got %.9g want %.9g err %.3g" % (what, name, got, want, err))
    # ---- gradients
    gworst = {}
    for name in run.grads.slots:
        if not run.grads.slots[name][1]:
            continue
        want, got = ref["grads"][name], out[name].astype(np.float64)
        assert want.shape == shapes[name] == got.shape
        scale = np.abs(want).max()
        err = np.abs(got - want)
        gworst[name] = float(err.max() / scale) if scale > 0 else float(err.max())
        print("%s grad %-11s max|ref| %.6g err/max|ref| %.3g, %d of %d exactly zero in the reference" % (
            what, name, scale, gworst[name], int((want == 0).sum()), want.size))
    for name, err in worst.items():
        assert err <= TOL, (what, name, err)
    for name, err in gworst.items():
        want, got = ref["grads"][name], out[name]
        assert np.isfinite(got).all(), (what, name)
        assert (got[want == 0] == 0).all(), (what, name, "an element that is exactly 0 in the reference is not")
        assert err <= TOL, (what, name, err)
    print("%s WORST stat %.3g (%s) grad %.3g (%s)" % (what, max(worst.values()), max(worst, key=worst.get),
                                                     max(gworst.values()), max(gworst, key=gworst.get)))


def check_plants(c, ref):
    """the planted edges are what they claim to be (decided by the float64 reference)"""
    p, K, B = c["plants"], c["K"], c["B"]
    lab = ref["objectness_label"]
    ps, empty = p["scene"], p["empty_scene"]
    if empty is not None:
        assert (ref["object_assignment"][empty] == 0).all() and not lab[empty].any()
        assert not c["box_label_mask"][empty].any()
    if c["no_positive"]:
        assert not lab.any() and ref["stats"]["obj_count"] == 0
        for name in ("g_h_scores", "g_h_resn", "g_s_scores", "g_s_resn", "g_sem", "g_vote"):
            assert not ref["grads"].get(name, np.zeros(1)).any(), name
        return
    mask = ref["objectness_mask"]
    n = lab[ps].size
    if n >= 30:  # all three objectness classes are populated
        assert lab[ps].sum() > n // 5 and (mask[ps] == 0).sum() > n // 5
        assert ((mask[ps] == 1) & (lab[ps] == 0)).sum() > n // 5
    for b in (b for b in range(B) if b != empty):
        assert lab[b, p["kq"]] == 1 and ref["gt_nearest"][b, p["g1"]] == p["kq"]
        if p["g2"] is not None:
            assert ref["gt_nearest"][b, p["g2"]] == p["kq"] and c["box_label_mask"][b, p["g2"]] == 1
    assert lab[ps, p["pa"]] == 1 and lab[ps, p["pb"]] == 1
    if K > 1:
        assert ref["clamped"][ps, p["pb"]].all() and ref["clamped"].mean() < 0.1
    if c["NH"] > 1 and K > 2:
        assert ref["boxes"][ps, p["pc"], 6] > 0  # -(angle - 2 pi): the wrap was taken


def _fused(monkeypatch, host=None):
    load_pkg()
    fused = importlib.import_module("3dioumatch_amd.votenet.fused_loss")
    if host is not None:
        monkeypatch.setattr(fused, "_HOST_BUILD", host)
    return fused


def _one(name, consistency, no_positive, dev, monkeypatch, host=None):
    scale = 0.37 if name in SCALED else 1.0
    c = build(name, consistency, no_positive)
    ref = reference(name, consistency, no_positive, scale)
    check_plants(c, ref)
    with monkeypatch.context() as mp:
        fused = _fused(mp, host)
        run = run_case(fused, dev, c, scale, mp)
        what = "%s%s%s" % (name, " consistency" if consistency else "", " no-positive" if no_positive else "")
        check_case(fused, c, run, ref, what)
    return fused, c, run


MODES = [pytest.param(False, id="supervised"), pytest.param(True, id="consistency")]


def _cases():
    return [pytest.param(n, cons, id="%s-%s" % (n, "consistency" if cons else "supervised"))
            for n in CASES for cons in (False, True) if not cons or n in CONSISTENCY_CASES]


# ------------------------------------------------------------------ CPU leg: builder, margins, reference
@pytest.mark.parametrize("name,consistency", _cases())
def test_host_build_against_float64(name, consistency, host_build, monkeypatch):  # noqa: F811
    _one(name, consistency, False, torch.device("cpu"), monkeypatch, host_build)


@pytest.mark.parametrize("consistency", MODES)
def test_host_build_no_positive_anywhere(consistency, host_build, monkeypatch):  # noqa: F811
    """no positive proposal and every vote_label_mask zero: both normalisers are 1e-6 and every
    positive-only term and gradient is exactly 0"""
    _one("one_lane_over", consistency, True, torch.device("cpu"), monkeypatch, host_build)


def test_builder_layouts():
    """the strided cases hand the binding the views the detector passes: (B, K, C) over (B, C, K) memory"""
    t = tensors(build("limits_wide_rows"), torch.device("cpu"))
    B, K, NS = 2, 513, 40
    assert t["sem"].stride() == (K * 37, 1, K) and t["s_resn"].stride() == (NS * 3 * K, 1, 3 * K, K)
    assert t["iou_lab"].min() == 0 and t["iou_lab"].max() == 1 and t["iou_assign"].dtype == torch.int32
    assert tensors(build("second_block"), torch.device("cpu"))["sem"].is_contiguous()


# ------------------------------------------------------------------ the semi-supervised node
SEMI = [pytest.param("second_block", 2, id="second_block-2-labeled"),
        pytest.param("one_lane_over", 1, id="one_lane_over-1-labeled")]
SEMI_WEIGHT = 2.0  # train.py:333; a power of two: the in-kernel grad_scale and autograd's product round alike
HEAD_KEYS = {"objectness_scores": "obj", "center": "center", "heading_scores": "h_scores",
             "heading_residuals_normalized": "h_resn", "size_scores": "s_scores",
             "size_residuals_normalized": "s_resn", "sem_cls_scores": "sem", "iou_scores": "iou",
             "iou_scores_jitter": "iou_jit", "vote_xyz": "vote_xyz"}
SUPERVISED_ONLY = ("iou_scores", "iou_scores_jitter", "vote_xyz", "objectness_scores")


def _semi_end_points(c, t, ln):
    """end_points of a semi-supervised step out of a supervised case: every scene's head outputs as leaf
    tensors, the case's labels (the first ln scenes are the labeled ones), and as pseudo labels the case's own
    labels of the remaining scenes"""
    ep = {key: t[name].detach().requires_grad_(True) for key, name in HEAD_KEYS.items()}
    ep.update({k: t[k] for k in ("center_label", "box_label_mask", "heading_class_label", "heading_residual_label",
                                 "size_class_label", "size_residual_label", "sem_cls_label", "vote_label",
                                 "vote_label_mask", "seed_inds", "seed_xyz", "jitter_center", "jitter_size",
                                 "jitter_heading")})
    ep["aggregated_vote_xyz"] = t["agg_xyz"]
    for k in ("center_label", "box_label_mask", "heading_class_label", "heading_residual_label", "size_class_label",
              "size_residual_label", "sem_cls_label"):
        ep["unlabeled_" + k] = t[k][ln:].clone()
    return ep


def _bits(x):
    x = x.detach().cpu().contiguous()
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def semi_case(fused, dev, name, ln, monkeypatch):
    """One gradient buffer for both losses (get_semi_loss_fused) against the two separate nodes
    (get_labeled_loss_fused on the labeled scenes + SEMI_WEIGHT * get_pseudo_detection_loss_fused) on the same
    inputs: (end_points, loss) of each, after backward, and the launches of the first."""
    c = build(name)
    assert c["jitter"] and 0 < ln < c["B"]
    t = tensors(c, dev)
    cfg = _Config(t["mean_size"])
    calls = []
    real_launch = fused._launch
    monkeypatch.setattr(fused, "_launch", lambda n, a, d: (calls.append(n), real_launch(n, a, d)))
    monkeypatch.setattr(fused, "_scene_iou", lambda boxes, gt_boxes: (t["iou_lab"][:ln], t["iou_assign"][:ln]))
    one = _semi_end_points(c, t, ln)
    loss_one, one = fused.get_semi_loss_fused(one, cfg, ln, SEMI_WEIGHT)
    launched = list(calls)
    loss_one.backward()
    two = _semi_end_points(c, t, ln)
    labeled, two = fused.get_labeled_loss_fused(two, cfg, slice(0, ln))
    unlabeled, two = fused.get_pseudo_detection_loss_fused(two, ln, cfg)
    loss_two = labeled + unlabeled * SEMI_WEIGHT
    loss_two.backward()
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return (one, loss_one), (two, loss_two), launched


def check_semi(fused, name, ln, result):
    (one, loss_one), (two, loss_two), launched = result
    assert launched == ["votenet_loss_decode", "votenet_loss_forward_backward", "votenet_loss_forward_backward"]
    assert torch.equal(_bits(loss_one), _bits(loss_two)) and torch.equal(_bits(one["loss"]), _bits(loss_one))
    logged = list(fused._STAT_KEYS) + list(fused._JITTER_KEYS) + list(fused._CONSISTENCY_KEYS)
    for key in logged + ["detection_loss", "unlabeled_detection_loss"]:
        assert not one[key].requires_grad
        assert torch.equal(_bits(one[key]), _bits(two[key])), (name, key, float(one[key]), float(two[key]))
    for key in ("objectness_label", "objectness_mask", "object_assignment", "pred_bbox", "unlabeled_objectness_label",
                "unlabeled_objectness_mask", "unlabeled_object_assignment", "unlabeled_center_label"):
        assert one[key].shape == two[key].shape and torch.equal(_bits(one[key]), _bits(two[key])), (name, key)
    assert one["objectness_label"].shape[0] == ln and one["pred_bbox"].shape[1] == one["center"].shape[1]
    assert int(one["objectness_label"].sum()) + int(one["unlabeled_objectness_label"].sum()) > 0
    for key in HEAD_KEYS:
        got, want = one[key].grad.cpu(), two[key].grad.cpu()
        assert got.shape == one[key].shape and bool(torch.isfinite(got).all()), (name, key)
        one_class = key == "heading_scores" and got.shape[2] == 1  # (cross entropy over one class: no gradient)
        # (equal as numbers: the kernels write -0.0 where a factor is negative, and autograd's sum of the two
        # nodes' zero-padded slices turns that into +0.0; every other element has the same bits)
        assert torch.equal(got, want), (name, key, float((got - want).abs().max()))
        assert torch.equal(_bits(got)[got != 0], _bits(want)[want != 0]), (name, key)
        if key in SUPERVISED_ONLY:
            assert not got[ln:].any(), (name, key, "a gradient on the rows of an unlabeled scene")
        elif not one_class:
            assert got[ln:].any(), (name, key)  # (the consistency rows are there)


@pytest.mark.parametrize("name,ln", SEMI)
def test_host_build_semi_node_equals_two_nodes(name, ln, host_build, monkeypatch):  # noqa: F811
    """the semi-supervised node (both modes of the pass builder writing the rows of ONE zero-filled gradient
    buffer per head output, the consistency rows scaled in the kernel) is bit-equal to the two separate nodes:
    loss, every logged key, labels, pred_bbox, the gradient of every head output; the unlabeled rows of
    iou_scores, iou_scores_jitter, vote_xyz and objectness_scores get exactly zero.  Shapes: a partial second
    proposal block with contiguous head outputs, and two votes per seed with strided ones."""
    fused = _fused(monkeypatch, host_build)
    check_semi(fused, name, ln, semi_case(fused, torch.device("cpu"), name, ln, monkeypatch))


# ------------------------------------------------------------------ GPU leg: the kernels
@pytest.mark.gpu
@pytest.mark.parametrize("name,consistency", _cases())
def test_kernels_against_float64(name, consistency, monkeypatch):
    _one(name, consistency, False, torch.device("cuda:0"), monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("consistency", MODES)
def test_kernels_no_positive_anywhere(consistency, monkeypatch):
    _one("one_lane_over", consistency, True, torch.device("cuda:0"), monkeypatch)


@pytest.mark.gpu
def test_entry_points_reject_bad_arguments(monkeypatch):
    """G = 257, K = 2049, NI not in {1, NC}, consistency with S != 0: refused by all three entry points
    (hipErrorInvalidValue, 0 scratch floats); partials = NULL: refused by votenet_loss_forward_backward.
    Nothing is launched: every output buffer still holds its sentinel.  The arguments are those of a real
    pass (`one_lane_over`: NC = 18, S = 257), every pointer a live device buffer of that pass."""
    dev = torch.device("cuda:0")
    fused, c, run = _one("one_lane_over", False, False, dev, monkeypatch)
    L = importlib.import_module("3dioumatch_amd._lib")
    for arena in run.own.values():
        arena.buf.fill_(SENTINEL[arena.buf.dtype])
    stream = L.current_stream_ptr(dev)
    assert L.lib.votenet_loss_scratch_floats(ctypes.byref(run.args)) == run.own["f"].slots["partials"][1] > 0
    changes = [dict(G=257), dict(K=2049), dict(NI=5), dict(NI=0), dict(consistency=1)]
    for change in changes:
        a = type(run.args).from_buffer_copy(run.args)
        for field, value in change.items():
            setattr(a, field, value)
        assert L.lib.votenet_loss_scratch_floats(ctypes.byref(a)) == 0, change
        assert L.lib.votenet_loss_decode(ctypes.byref(a), stream) == INVALID, change
        assert L.lib.votenet_loss_forward_backward(ctypes.byref(a), stream) == INVALID, change
    a = type(run.args).from_buffer_copy(run.args)
    a.partials = None
    assert L.lib.votenet_loss_forward_backward(ctypes.byref(a), stream) == INVALID
    torch.cuda.synchronize()
    for key, arena in run.own.items():
        arena.check("rejected " + key, written=False)


@pytest.mark.gpu
@pytest.mark.parametrize("name,ln", SEMI)
def test_kernels_semi_node_equals_two_nodes(name, ln, monkeypatch):
    """as test_host_build_semi_node_equals_two_nodes, on the kernels (no atomics in them: the same bits)"""
    fused = _fused(monkeypatch)
    check_semi(fused, name, ln, semi_case(fused, torch.device("cuda:0"), name, ln, monkeypatch))
