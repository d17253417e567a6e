"""Regenerate tests/golden/view_stats_ref.npz with the REFERENCE's own
models/loss_helper_unlabeled.py:get_unlabeled_loss and config_dict['view_stats'] = True (build
container only):

    python tests/golden/make_view_stats_golden.py

As tests/golden/make_unlabeled_golden.py, the reference module is imported from /root/reference and
run on the CPU (Tensor.cuda patched to the identity); as tests/golden/make_iou_labels_golden.py, its
CUDA-only box3d_iou_batch_gpu is the oracle's 3-D IoU (pinned bit-for-bit to the reference's compiled
iou3d_cpu.cpp).  Stored per dataset config (ScanNet: axis-aligned, SUN RGB-D: 12 heading bins):
  inputs  : end_points (student outputs, augmentation, the box labels of ALL rows -- unlabeled ones
            in the teacher's frame) and the teacher's outputs
  outputs : the twelve view_stats scalars and unlabeled_iou_labels (S,K)
The inputs are drawn so that the numbers say something: IoU labels over (0, 1), GT boxes covered
and missed at 0.25 and at 0.5, one unlabeled scene without a GT box, one in which no proposal passes
the thresholds, more than 64 survivors of the thresholds in every other (the reference's argsort is
not stable: which non-passing proposals fill the free slots would reach its NMS) -- and seeds are
skipped until every coverage maximum, vote distance, best-vs-second
IoU gap of a kept slot and filter score is at least 1e-3 (scores: 1e-5) away from where an ulp
could flip it.
Only data is stored.
"""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

B_LAB, B_UNL, K, G = 2, 4, 128, 64
EMPTY_SCENE, SILENT_SCENE = 1, 2          # unlabeled scenes: no GT box / no proposal passes
STAT_KEYS = ["unlabeled_pred_iou_value", "unlabeled_pred_iou_obj_value", "unlabeled_iou_acc",
             "unlabeled_iou_obj_acc", "final_iou_avg_value", "final_iou_avg_obj_value", "final_cls_value",
             "final_cls_obj_value", "final_coverage_0.25_value", "final_coverage_0.5_value",
             "true_unlabeled_obj_acc", "unlabeled_obj_acc"]
GT_KEYS = ["center_label", "heading_class_label", "heading_residual_label", "size_class_label",
           "size_residual_label", "sem_cls_label", "box_label_mask"]


def make_inputs(cfg, seed):
    g = torch.Generator().manual_seed(seed)
    b = B_LAB + B_UNL
    nh, ns, nc = cfg.num_heading_bin, cfg.num_size_cluster, cfg.num_class
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    u = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    datamod = importlib.import_module("3dioumatch_amd.votenet.data")
    batch = datamod.make_batch(b, 1024, cfg, seed=seed, num_objects=10)
    labels = {k: batch[k].clone() for k in GT_KEYS}
    e = B_LAB + EMPTY_SCENE
    labels["box_label_mask"][e] = 0
    labels["center_label"][e] = u(G, 3) * 4          # garbage behind the mask: must be ignored
    n_obj = labels["box_label_mask"].sum(1).long()
    # teacher proposals around the GT boxes of their scene: centre noise from tight to loose so the
    # IoU labels spread over (0, 1); every 9th far away
    pick = (u(b, K) * n_obj.clamp(min=1).unsqueeze(1)).long()
    gt_center = torch.gather(labels["center_label"], 1, pick.unsqueeze(-1).expand(-1, -1, 3))
    spread = 0.02 + 0.5 * u(b, K, 1) ** 2
    center = gt_center + r(b, K, 3) * spread
    center[:, ::9] += 4.0
    s_cls = torch.gather(labels["size_class_label"], 1, pick)
    h_cls = torch.gather(labels["heading_class_label"], 1, pick)
    # (the losses' inputs that no statistic reads are zeros or one-hot: a small, compressible file)
    size_scores = torch.zeros(b, K, ns).scatter_(2, s_cls.unsqueeze(-1), 5.0)
    heading_scores = torch.zeros(b, K, nh).scatter_(2, h_cls.unsqueeze(-1), 5.0)
    gt_sres = torch.gather(labels["size_residual_label"], 1, pick.unsqueeze(-1).expand(-1, -1, 3))
    size_res = torch.zeros(b, K, ns, 3).scatter_(2, s_cls.view(b, K, 1, 1).expand(-1, -1, 1, 3),
                                                 (gt_sres + r(b, K, 3) * 0.1).unsqueeze(2))
    gt_hres = torch.gather(labels["heading_residual_label"], 1, pick)
    heading_res = torch.zeros(b, K, nh).scatter_(2, h_cls.unsqueeze(-1), (gt_hres + r(b, K) * 0.1).unsqueeze(-1))
    confident = u(b, K) < 0.75
    confident[B_LAB + SILENT_SCENE] = False
    # class: mostly the GT's, every 5th another one (final_cls < 1)
    gt_sem = torch.gather(labels["sem_cls_label"], 1, pick)
    cls = torch.where(torch.arange(K).unsqueeze(0) % 5 == 3, (gt_sem + 1) % nc, gt_sem)
    sem = r(b, K, nc) + 9 * torch.nn.functional.one_hot(cls, nc) * confident.unsqueeze(-1)
    ema = {
        "center": center,
        "aggregated_vote_xyz": center + r(b, K, 3) * 0.12,
        "objectness_scores": torch.stack([-(3 + u(b, K) * 3), 3 + u(b, K) * 3], 2)
        * torch.where(confident, 1.0, 0.1).unsqueeze(-1),
        "sem_cls_scores": sem,
        "heading_scores": heading_scores,
        "heading_residuals": heading_res,
        "size_scores": size_scores,
        "size_residuals": size_res,
        "iou_scores": r(b, K, nc) * 1.2 + torch.where(confident, 1.0, -0.5).unsqueeze(-1),
    }
    ep = {
        "supervised_mask": torch.tensor([1] * B_LAB + [0] * B_UNL),
        "center": center + r(b, K, 3) * 0.2,
        "objectness_scores": r(b, K, 2),
        "heading_scores": torch.zeros(b, K, nh),
        "heading_residuals_normalized": torch.zeros(b, K, nh),
        "size_scores": torch.zeros(b, K, ns),
        "size_residuals_normalized": torch.zeros(b, K, ns, 3),
        "sem_cls_scores": torch.zeros(b, K, nc),
        "flip_x_axis": torch.randint(0, 2, (b,), generator=g),
        "flip_y_axis": torch.randint(0, 2, (b,), generator=g),
        "rot_angle": (u(b) - 0.5) * (np.pi / 18),
        "scale": (u(b, 1, 3) * 0.3 + 0.85),
    }
    c, s = torch.cos(ep["rot_angle"]), torch.sin(ep["rot_angle"])
    z, o = torch.zeros(b), torch.ones(b)
    ep["rot_mat"] = torch.stack([c, -s, z, s, c, z, z, z, o], 1).view(b, 3, 3)
    # the student's votes: the teacher's centres in the student's frame, jittered
    stud = center.clone()
    stud[:, :, 0] = torch.where(ep["flip_x_axis"].bool().unsqueeze(1), -stud[:, :, 0], stud[:, :, 0])
    stud[:, :, 1] = torch.where(ep["flip_y_axis"].bool().unsqueeze(1), -stud[:, :, 1], stud[:, :, 1])
    ep["aggregated_vote_xyz"] = torch.bmm(stud, ep["rot_mat"].transpose(1, 2)) * ep["scale"] + r(b, K, 3) * 0.15
    ep.update(labels)
    return ep, ema


def decode_gt(labels, cfg):
    """losses._gt_boxes in numpy-free torch (the GT half of compute_iou_labels)."""
    center = torch.where((1 - labels["box_label_mask"]).unsqueeze(-1).bool(), torch.full_like(
        labels["center_label"], -1000), labels["center_label"])
    size = cfg.class2size_gpu(labels["size_class_label"], labels["size_residual_label"])
    angle = cfg.class2angle_gpu(labels["heading_class_label"], labels["heading_residual_label"])
    return torch.cat([center, size, -angle[:, :, None]], 2)


def margins_ok(oracle, cfg, ep, ema, out, config_dict):
    """True when nothing the test compares sits within an ulp-flip of a threshold or a tie."""
    tail = slice(B_LAB, None)
    gt = decode_gt({k: ep[k][tail] for k in GT_KEYS}, cfg)
    pred = out["pred_bbox"].detach()          # the teacher's boxes (compute_iou_labels)
    pos = torch.softmax(ema["objectness_scores"][tail], 2)[:, :, 1]
    sem = torch.softmax(ema["sem_cls_scores"][tail], 2)
    max_cls, argmax_cls = sem.max(2)
    iou_pred = torch.gather(torch.sigmoid(ema["iou_scores"][tail]), 2, argmax_cls.unsqueeze(-1)).squeeze(-1)
    for v, t in ((pos, 0.9), (max_cls, 0.9), (iou_pred, 0.25)):
        if bool(((v - t).abs() < 1e-5).any()):
            return "score"
    mask = (pos > 0.9) & (max_cls > 0.9) & (iou_pred > 0.25)
    key = pos * max_cls * mask
    if any(int(mask[i].sum()) != len(set(key[i][mask[i]].tolist())) for i in range(B_UNL)):
        return "key tie"
    # more than 64 survivors in every scene but the silent one: the reference's argsort is not
    # stable, and which non-passing proposals fill the remaining slots would matter to its NMS
    passing = mask.sum(1)
    if any(int(passing[i]) <= 64 for i in range(B_UNL) if i != SILENT_SCENE):
        return "too few survivors"
    inds = torch.argsort(key, dim=1, descending=True, stable=True)[:, :64]
    kept = out["unlabeled_box_label_mask"].bool()
    for i in range(B_UNL):
        m = oracle.boxes_iou3d(pred[i].numpy(), gt[i].numpy())          # (K,G)
        srt = np.sort(m[inds[i][kept[i]].numpy()], 1)                   # the kept slots' GT match
        if bool(((srt[:, -1] > 0) & (srt[:, -1] - srt[:, -2] < 1e-3)).any()):
            return "assignment gap"
        rev = oracle.boxes_iou3d(gt[i].numpy(), pred[i].numpy())        # (G,K)
        cov = (rev[:, inds[i].numpy()] * kept[i].numpy()[None, :]).max(1)
        if bool((np.abs(cov - 0.25) < 1e-3).any() or (np.abs(cov - 0.5) < 1e-3).any()):
            return "coverage"
    d = torch.cdist(ema["aggregated_vote_xyz"][tail], gt[:, :, :3]).min(2)[0]
    if bool(((d - 0.3).abs() < 1e-3).any()):
        return "teacher vote"
    stud = torch.where((1 - ep["box_label_mask"][tail]).unsqueeze(-1).bool(), torch.tensor(-1000.0),
                       out["_student_gt"])
    d = torch.cdist(ep["aggregated_vote_xyz"][tail], stud).min(2)[0]
    if bool(((d - 0.3).abs() < 1e-3).any() or ((d - 0.6).abs() < 1e-3).any()):
        return "student vote"
    return None


def main():
    from oracle.oracle import Oracle
    o = Oracle(omp=True)
    for name in ("pcdet", "pcdet.ops", "pcdet.ops.iou3d_nms"):
        sys.modules[name] = types.ModuleType(name)
    iou_stub = types.ModuleType("pcdet.ops.iou3d_nms.iou3d_nms_utils")
    iou_stub.boxes_iou3d_gpu = lambda a, b: torch.from_numpy(o.boxes_iou3d(a.detach().numpy(), b.detach().numpy()))
    sys.modules["pcdet.ops.iou3d_nms.iou3d_nms_utils"] = iou_stub
    pc = types.ModuleType("pc_util")
    pc.bbox_corner_dist_measure = None
    sys.modules["pc_util"] = pc
    ap = types.ModuleType("models.ap_helper")

    def flip_axis_to_camera(pc):  # models/ap_helper.py:28-35
        pc2 = np.copy(pc)
        pc2[..., [0, 1, 2]] = pc2[..., [0, 2, 1]]
        pc2[..., 1] *= -1
        return pc2
    ap.flip_axis_to_camera = flip_axis_to_camera
    sys.modules["models.ap_helper"] = ap
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.cuda.FloatTensor = torch.FloatTensor
    # the product's data / config modules (synthetic labels and mean sizes); the package __init__
    # would load the HIP library, so the two modules are loaded from their files
    pkg = types.ModuleType("3dioumatch_amd")
    pkg.__path__ = [os.path.join(ROOT, "3dioumatch_amd")]
    sys.modules["3dioumatch_amd"] = pkg
    vn = types.ModuleType("3dioumatch_amd.votenet")
    vn.__path__ = [os.path.join(ROOT, "3dioumatch_amd", "votenet")]
    sys.modules["3dioumatch_amd.votenet"] = vn
    cfgmod = importlib.import_module("3dioumatch_amd.votenet.config")
    importlib.import_module("3dioumatch_amd.votenet.data")
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REF, "utils"))
    ref = importlib.import_module("models.loss_helper_unlabeled")

    out = {}
    for tag, cfg in (("scannet", cfgmod.scannet_config()), ("sunrgbd", cfgmod.sunrgbd_config())):
        class RefConfig(object):  # what the reference's dataset configs provide, numpy in float64
            num_class, num_heading_bin, num_size_cluster = cfg.num_class, cfg.num_heading_bin, cfg.num_size_cluster
            mean_size_arr = cfg.mean_size_arr.astype(np.float64)
            class2angle = staticmethod(cfg.class2angle)
            class2angle_gpu = staticmethod(cfg.class2angle_gpu)
            angle2class_gpu = staticmethod(cfg.angle2class_gpu)
            class2size_gpu = staticmethod(cfg.class2size_gpu)

            @staticmethod
            def class2size(pred_cls, residual):
                return cfg.mean_size_arr.astype(np.float64)[pred_cls, :] + residual
        config_dict = {"dataset_config": RefConfig, "unlabeled_batch_size": B_UNL, "dataset": tag,
                       "nms_iou": 0.25, "use_old_type_nms": False, "obj_threshold": 0.9,
                       "cls_threshold": 0.9, "use_lhs": True, "iou_threshold": 0.25,
                       "samecls_match": False, "view_stats": True}
        for seed in range(100, 1000):
            ep, ema = make_inputs(cfg, seed)
            inputs = ({k: v.clone() for k, v in ep.items()}, {k: v.clone() for k, v in ema.items()})
            loss, res = ref.get_unlabeled_loss({k: v.clone() for k, v in ep.items()},
                                               {k: v.clone() for k, v in ema.items()}, RefConfig, config_dict)
            res["_student_gt"] = ref.trans_center(ep["center_label"][B_LAB:], ep["flip_x_axis"][B_LAB:],
                                                  ep["flip_y_axis"][B_LAB:], ep["rot_mat"][B_LAB:],
                                                  ep["scale"][B_LAB:])
            why = margins_ok(o, cfg, ep, ema, res, config_dict)
            stats = {k: float(res[k]) for k in STAT_KEYS}
            kept = res["unlabeled_box_label_mask"].sum(1).tolist()
            # something to see: covered and missed at both thresholds, kept boxes in the other scenes
            if why is None and not (0 < stats["final_coverage_0.5_value"] < stats["final_coverage_0.25_value"]
                                    < float(ep["box_label_mask"][B_LAB:].sum() / ep["box_label_mask"].sum())):
                why = "coverage trivial"
            if why is None and (kept[SILENT_SCENE] != 0 or min(kept[i] for i in range(B_UNL) if i != SILENT_SCENE) == 0):
                why = "kept boxes"
            if why is None:
                break
            print(tag, "seed", seed, "skipped:", why)
        else:
            raise SystemExit("no seed with safe margins")
        for k, v in inputs[0].items():
            out["%s_in_ep::%s" % (tag, k)] = v.numpy()
        for k, v in inputs[1].items():
            out["%s_in_ema::%s" % (tag, k)] = v.numpy()
        for k in STAT_KEYS:
            out["%s_stat::%s" % (tag, k)] = np.float64(stats[k])
        out[tag + "_iou_labels"] = res["unlabeled_iou_labels"].numpy()
        out[tag + "_loss"] = loss.detach().numpy()
        iou = res["unlabeled_iou_labels"]
        print(tag, "seed", seed, "kept per scene", kept, "IoU labels > 0: %d of %d, mean %.3f" % (
            int((iou > 0).sum()), iou.numel(), float(iou.mean())))
        print("   ", ", ".join("%s %.4f" % (k, v) for k, v in stats.items()))
    path = os.path.join(HERE, "view_stats_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path) // 1024, "KB")


if __name__ == "__main__":
    main()
