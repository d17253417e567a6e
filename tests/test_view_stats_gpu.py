"""`view_stats` on the MI355X: the two launches of lhs_pseudo_stats (csrc/lhs_stats.hip, through
pseudo_nms.pseudo_label_stats_gpu) against the reference's golden vectors and against the tensor
mirror on the GPU (same IoU kernels: identical IoU labels and GT assignments, sums within rounding),
and the captured stage-2 step with the flag: logging only, bit for bit."""
import importlib

import numpy as np
import pytest
import torch

from conftest import golden, load_pkg
from test_view_stats import COUNT_KEYS, LABEL_KEYS, STAT_KEYS, golden_inputs, run_loss

pytestmark = pytest.mark.gpu


def _mods():
    load_pkg()
    return (importlib.import_module("3dioumatch_amd.votenet"),
            importlib.import_module("3dioumatch_amd.votenet.losses_unlabeled"))


@pytest.mark.parametrize("tag", ["scannet", "sunrgbd"])
def test_kernel_matches_reference(tag):
    V, U = _mods()
    g = golden("view_stats_ref.npz")
    cfg = V.scannet_config() if tag == "scannet" else V.sunrgbd_config()
    ep, ema = golden_inputs(g, tag, "cuda:0")
    labels_before = {k: ep[k].clone() for k in U.GT_KEYS}
    _, out = run_loss(U, cfg, tag, ep, ema, True)
    for k in STAT_KEYS:
        got, want = float(out[k]), float(g["%s_stat::%s" % (tag, k)])
        assert abs(got - want) <= 1e-4, (k, got, want)
        if k in COUNT_KEYS:
            assert got == np.float32(want), (k, got, want)
    np.testing.assert_allclose(out["unlabeled_iou_labels"].cpu().numpy(), g[tag + "_iou_labels"], rtol=0,
                               atol=1e-4)
    for k, v in labels_before.items():
        assert torch.equal(ep[k], v), k


def _random_case(V, tag, s, k, ni, seed):
    """Teacher proposals around the GT boxes of their scene (IoU labels over (0, 1)), a chosen half
    passing the thresholds with all-different margins; scene 1 without GT boxes, scene 2 without a
    survivor (when there are three scenes or more)."""
    cfg = V.scannet_config() if tag == "scannet" else V.sunrgbd_config()
    g = torch.Generator().manual_seed(seed)
    lab = 2
    b = lab + s
    nh, ns, nc = cfg.num_heading_bin, cfg.num_size_cluster, cfg.num_class
    semi = V.make_semi_batch(lab, s, 1024, cfg, seed=seed, num_objects=10, unlabeled_labels=True)
    if s >= 3:
        semi["box_label_mask"][lab + 1] = 0
    r = lambda *sh: torch.randn(*sh, generator=g)  # noqa: E731
    n_obj = semi["box_label_mask"].sum(1).long().clamp(min=1)
    pick = (torch.rand(b, k, generator=g) * n_obj.unsqueeze(1)).long()
    center = torch.gather(semi["center_label"], 1, pick.unsqueeze(-1).expand(-1, -1, 3))
    center = center + r(b, k, 3) * (0.02 + 0.5 * torch.rand(b, k, 1, generator=g) ** 2)
    s_cls = torch.gather(semi["size_class_label"], 1, pick)
    size_scores = r(b, k, ns).scatter_(2, s_cls.unsqueeze(-1), 5.0)
    size_res = r(b, k, ns, 3) * 0.1
    size_res.scatter_add_(2, s_cls.view(b, k, 1, 1).expand(-1, -1, 1, 3), torch.gather(
        semi["size_residual_label"], 1, pick.unsqueeze(-1).expand(-1, -1, 3)).unsqueeze(2))
    h_cls = torch.gather(semi["heading_class_label"], 1, pick)
    heading_scores = r(b, k, nh).scatter_(2, h_cls.unsqueeze(-1), 5.0)
    sure = torch.rand(b, k, generator=g) < 0.5
    if s >= 3:
        sure[lab + 2] = False
    obj = r(b, k, 2)
    margin = 2.5 + 6.0 * torch.stack([torch.randperm(k, generator=g) for _ in range(b)]).float() / k
    obj[..., 1] = torch.where(sure, obj[..., 0] + margin, obj[..., 1])
    top = torch.gather(semi["sem_cls_label"], 1, pick)
    # class probability 1.0f exactly: the sort key is the objectness alone, whose margins are all
    # different (keys one ulp apart could legitimately sort differently in the two filters)
    sem = torch.where(sure.unsqueeze(-1), r(b, k, nc).scatter(2, top.unsqueeze(-1), 30.0), r(b, k, nc))
    ema = {"center": center, "aggregated_vote_xyz": center + r(b, k, 3) * 0.1, "heading_scores": heading_scores,
           "heading_residuals": r(b, k, nh) * 0.1, "size_scores": size_scores, "size_residuals": size_res,
           "objectness_scores": obj, "sem_cls_scores": sem,
           "iou_scores": r(b, k, ni) + torch.where(sure, 2.0, -2.0).unsqueeze(-1)}
    ep = {key: semi[key] for key in ("flip_x_axis", "flip_y_axis", "rot_mat", "rot_angle", "scale",
                                     "supervised_mask") + tuple(importlib.import_module(
                                         "3dioumatch_amd.votenet.data").BOX_LABEL_KEYS)}
    ep.update({"center": center + r(b, k, 3) * 0.2, "aggregated_vote_xyz": center + r(b, k, 3) * 0.3,
               "objectness_scores": r(b, k, 2), "heading_scores": r(b, k, nh),
               "heading_residuals_normalized": r(b, k, nh) * 0.3, "size_scores": r(b, k, ns),
               "size_residuals_normalized": r(b, k, ns, 3) * 0.3, "sem_cls_scores": r(b, k, nc)})
    dev = torch.device("cuda:0")
    ep = {key: v.to(dev) for key, v in ep.items()}
    ep["labeled_num"] = lab
    return cfg, ep, {key: v.to(dev) for key, v in ema.items()}


@pytest.mark.parametrize("tag,s,k,ni", [("scannet", 1, 64, "nc"), ("sunrgbd", 3, 256, "1"),
                                        ("scannet", 8, 256, "nc"), ("sunrgbd", 8, 1024, "nc"),
                                        ("scannet", 3, 1024, "1"), ("sunrgbd", 1, 256, "nc")])
def test_kernel_matches_tensor_mirror(tag, s, k, ni, monkeypatch):
    V, U = _mods()
    losses = importlib.import_module("3dioumatch_amd.votenet.losses")
    P = importlib.import_module("3dioumatch_amd.votenet.pseudo_nms")
    cfg0 = V.scannet_config() if tag == "scannet" else V.sunrgbd_config()
    cfg, ep, ema = _random_case(V, tag, s, k, 1 if ni == "1" else cfg0.num_class, seed=s * 7 + k)
    outs = []
    for flag in ("0", "1"):  # tensor mirror (GPU IoU kernels), then the fused path with lhs_pseudo_stats
        monkeypatch.setenv("VOTENET_FUSED_PSEUDO_LABELS", flag)
        outs.append(run_loss(U, cfg, tag, ep, ema, True))
    (l0, e0), (l1, e1) = outs
    for key in ("unlabeled_box_label_mask", "unlabeled_sem_cls_label"):
        assert torch.equal(e0[key].long(), e1[key].long()), key
    if s >= 3:
        assert int(e1["unlabeled_box_label_mask"][2].sum()) == 0
    assert int(e1["unlabeled_box_label_mask"].sum()) > 0
    assert torch.equal(e0["unlabeled_iou_labels"], e1["unlabeled_iou_labels"])
    iou = e1["unlabeled_iou_labels"]
    assert float(iou.max()) > 0.5 and int(((iou > 0) & (iou < 0.5)).sum()) > 0
    for key in STAT_KEYS:
        a, c = float(e0[key]), float(e1[key])
        assert abs(a - c) <= 1e-5 * abs(a) + 1e-7, (key, a, c)
    # the GT index of every IoU label: the kernel's == compute_iou_labels' (scene_max_kernel)
    lab = ep["labeled_num"]
    tail = slice(lab, None)
    gt = {key: ep[key] for key in U.GT_KEYS}
    _, _, assign = losses.compute_iou_labels(
        dict(gt), tail, ema["aggregated_vote_xyz"][tail], ema["center"][tail], ema["sem_cls_scores"][tail],
        ema["objectness_scores"][tail], ema["heading_scores"][tail], ema["heading_residuals"][tail],
        ema["size_scores"][tail], ema["size_residuals"][tail], {"dataset_config": cfg})
    teacher = [ema[key][tail] for key in ("objectness_scores", "sem_cls_scores", "iou_scores", "heading_scores",
                                          "heading_residuals", "size_scores", "size_residuals", "center",
                                          "aggregated_vote_xyz")]
    aug = [ep[key][tail] for key in ("flip_x_axis", "flip_y_axis", "rot_mat", "scale")]
    cd = U.default_config_dict(cfg)
    direct = P.pseudo_label_stats_gpu(*teacher, cfg.mean_size(ep["center"].device), e1["unlabeled_box_label_mask"],
                                      gt, lab, ep["objectness_scores"][tail], ep["aggregated_vote_xyz"][tail],
                                      *aug, cd["obj_threshold"], cd["cls_threshold"], cd["iou_threshold"],
                                      assignment=True)
    assert torch.equal(direct["unlabeled_iou_assignment"], assign)
    assert torch.equal(direct["unlabeled_iou_labels"], e1["unlabeled_iou_labels"])
    for key in STAT_KEYS:  # the same launch twice: the same bits (no float atomics)
        assert torch.equal(direct[key], e1[key]), key


def test_captured_step_flag_is_logging_only():
    """The captured stage-2 step at B = 4 + 8 from a common start, two steps with view_stats off and
    on: loss, flat gradient and parameters bit for bit; the replayed statistics == the same pass run
    eagerly on the graph's buffers afterwards."""
    V, U = _mods()
    step_mod = importlib.import_module("3dioumatch_amd.votenet.step")
    P = importlib.import_module("3dioumatch_amd.votenet.pseudo_nms")
    cfg = V.scannet_config()
    dev = torch.device("cuda:0")
    batches = [{k: v.to(dev) for k, v in V.make_semi_batch(4, 8, 20000, cfg, seed=s, num_objects=8,
                                                          unlabeled_labels=True).items()} for s in (5, 6)]
    results = []
    for flag in (False, True):
        cd = U.default_config_dict(cfg, unlabeled_batch_size=8, view_stats=flag)
        cd.update(obj_threshold=0.3, cls_threshold=0.03, iou_threshold=0.2)  # random weights: loosen
        runner = V.SemiSupervisedStep(cfg, dev, seed=4, graphs=True, config_dict=cd)
        torch.manual_seed(9)
        torch.cuda.manual_seed_all(9)
        views = [dict(bt) for bt in batches]
        runner.prefetch_geometry(views[0])
        out = []
        for i in range(2):
            if i + 1 < len(views):
                runner.prefetch_geometry(views[i + 1])
            loss, ep = runner(views[i])
            out.append((loss.detach().clone(), runner.flat_grad.detach().clone(),
                        step_mod.flat_params(runner.net).detach().clone(),
                        {k: ep[k].detach().clone() for k in LABEL_KEYS}))
        torch.cuda.synchronize()
        assert runner.graphs
        results.append((out, runner, ep))
    (off, _, ep_off), (on, runner, ep_on) = results
    for a, b in zip(off, on):
        assert torch.equal(a[0], b[0])
        assert torch.equal(a[1], b[1])
        assert torch.equal(a[2], b[2])
        for k in LABEL_KEYS:
            assert torch.equal(a[3][k], b[3][k]), k
    assert not any(k in ep_off for k in STAT_KEYS)
    assert int(ep_on["unlabeled_box_label_mask"].sum()) > 0
    # the statistics of the last replay, recomputed eagerly from the same static buffers
    lab, tail = 4, slice(4, None)
    ema = runner._ema_end_points
    gt = {k: runner._cur[k] for k in U.GT_KEYS}
    teacher = [ema[k][tail] for k in ("objectness_scores", "sem_cls_scores", "iou_scores", "heading_scores",
                                      "heading_residuals", "size_scores", "size_residuals", "center",
                                      "aggregated_vote_xyz")]
    aug = [runner._cur[k][tail] for k in ("flip_x_axis", "flip_y_axis", "rot_mat", "scale")]
    cd = runner.config_dict
    eager = P.pseudo_label_stats_gpu(*teacher, cfg.mean_size(dev), ep_on["unlabeled_box_label_mask"], gt, lab,
                                     ep_on["objectness_scores"][tail], ep_on["aggregated_vote_xyz"][tail], *aug,
                                     cd["obj_threshold"], cd["cls_threshold"], cd["iou_threshold"])
    for k in STAT_KEYS + ["unlabeled_iou_labels"]:
        assert torch.equal(eager[k], ep_on[k]), k
    assert float(ep_on["unlabeled_pred_iou_value"]) > 0
