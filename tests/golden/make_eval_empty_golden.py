"""Regenerate tests/golden/eval_parse_empty_ref.npz with the REFERENCE's models/ap_helper.py
parse_predictions for `remove_empty_box` and the 2-D NMS branch (build container only):

    python tests/golden/make_eval_empty_golden.py <checkout of the reference>

The reference's modules are imported from that checkout and run on the CPU, with its real
sunrgbd.sunrgbd_utils.extract_pc_in_box3d (scipy Delaunay per box).  Placeholders are registered
only for imports the parsed branches never touch (plotting / image packages absent here).  Only
data is stored: one set of seeded inputs (B = 2, K = 160, N = 4096, float32), the per-box point
counts of the reference, and per config variant the pred_mask and the kept lists as (class,
proposal index, confidence).

The generator checks its inputs and fails loudly otherwise: every decoded size >= 0.05 m, no point
within 1e-4 m of a face of any box (such points are redrawn), every scene has a non-empty box, the
counts contain 3, 4, 5 and 6 (hand-placed), between 2 % and 50 % of the boxes are empty, and the
closed-form count of tests/eval_empty_host.py equals the reference's triangulation everywhere.
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
B, K, N = 2, 160, 4096
MARGIN = 1e-4
HAND = (3, 4, 5, 6)        # boxes K-4 .. K-1 of scene 0 get exactly this many points


def decode(ep, cfg):
    h_cls = ep["heading_scores"].argmax(-1)
    h_res = torch.gather(ep["heading_residuals"], 2, h_cls.unsqueeze(-1)).squeeze(2)
    s_cls = ep["size_scores"].argmax(-1)
    s_res = torch.gather(ep["size_residuals"], 2, s_cls.view(B, K, 1, 1).expand(-1, -1, -1, 3)).squeeze(2)
    size = cfg.mean_size_arr.astype(np.float64)[s_cls.numpy()] + s_res.numpy()
    heading = s_cls.numpy() * 0.0
    for i in range(B):
        for j in range(K):
            heading[i, j] = cfg.class2angle(h_cls[i, j].numpy(), h_res[i, j].numpy())
    return size, heading.astype(np.float64)


def make_inputs(cfg, host, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    nh, ns, nc = cfg.num_heading_bin, cfg.num_size_cluster, cfg.num_class
    clumps = torch.rand(B, 10, 3, generator=g) * 5 - 2.5
    which = torch.randint(0, 10, (B, K), generator=g)
    center = torch.gather(clumps, 1, which.unsqueeze(-1).expand(-1, -1, 3)) + r(B, K, 3) * 0.25
    # one proposal in six strays from its clump, so that a share of the boxes is empty
    stray = torch.rand(B, K, generator=g) < 1.0 / 6.0
    center = center + stray.unsqueeze(-1) * r(B, K, 3) * 2.0
    # four isolated boxes (scene 0) that the draw leaves empty; points are placed in them by hand
    for q in range(len(HAND)):
        center[0, K - len(HAND) + q] = torch.tensor([8.0 + 3.0 * q, 8.0, 0.5])
    ep = {"center": center, "heading_scores": r(B, K, nh), "heading_residuals": r(B, K, nh) * 0.1,
          "size_scores": r(B, K, ns), "size_residuals": r(B, K, ns, 3) * 0.1,
          "sem_cls_scores": r(B, K, nc) * 2, "objectness_scores": r(B, K, 2) * 3,
          "iou_scores": r(B, K, nc)}
    size, heading = decode(ep, cfg)
    assert size.min() >= 0.05, "degenerate box: smallest decoded size %.4f" % size.min()

    def draw(count):
        w = torch.randint(0, 10, (count,), generator=g)
        return w, r(count, 3) * 0.45
    pc = torch.zeros(B, N, 4)
    for i in range(B):
        w, off = draw(N)
        pc[i, :, :3] = clumps[i][w] + off
    # hand-placed points: well inside the isolated boxes (|local coordinate| <= 0.2 * half extent)
    slot = 0
    for q, want in enumerate(HAND):
        j = K - len(HAND) + q
        c, s = np.cos(heading[0, j]), np.sin(heading[0, j])
        for _ in range(want):
            a, b_, e = (torch.rand(3, generator=g).numpy() * 2 - 1) * 0.2 * size[0, j] / 2
            pc[0, slot, :3] = center[0, j] + torch.tensor([c * a + s * b_, -s * a + c * b_, e], dtype=torch.float32)
            slot += 1
    center_np = center.numpy()
    for attempt in range(20):   # redraw the points that lie within the margin of a face
        near = (host.face_margin(pc.numpy(), center_np, size, heading) < MARGIN).any(1)   # (B,N)
        near[0, :slot] = False
        if not near.any():
            break
        for i in range(B):
            idx = np.nonzero(near[i])[0]
            w, off = draw(len(idx))
            pc[i, idx, :3] = clumps[i][w] + off
    margin = host.face_margin(pc.numpy(), center_np, size, heading)
    assert margin.min() >= MARGIN, "a point within %.1e m of a face survived the redraws" % MARGIN
    pc[:, :, 3] = pc[:, :, 2] - pc[:, :, 2].min(1, keepdim=True).values   # height, as the loaders add it
    ep["point_clouds"] = pc
    return ep, size, heading


def main():
    if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
        sys.exit(__doc__)
    ref = os.path.abspath(sys.argv[1])
    for name in ("utils.eval_det", "pc_util", "utils.pc_util", "cv2", "mayavi", "mayavi.mlab",
                 "pcdet", "pcdet.ops", "pcdet.ops.iou3d_nms", "pcdet.ops.iou3d_nms.iou3d_nms_utils"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["utils.eval_det"].eval_det_multiprocessing = None
    sys.modules["utils.eval_det"].get_iou_obb = None
    sys.modules["pc_util"].bbox_corner_dist_measure = None
    sys.modules["utils.pc_util"].random_sampling = None
    sys.modules["mayavi"].mlab = sys.modules["mayavi.mlab"]
    sys.modules["pcdet.ops.iou3d_nms.iou3d_nms_utils"].boxes_iou3d_gpu = None
    sys.path.insert(0, ref)
    sys.path.insert(0, os.path.join(ref, "utils"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    ap = importlib.import_module("models.ap_helper")
    extract = importlib.import_module("sunrgbd.sunrgbd_utils").extract_pc_in_box3d
    assert ap.extract_pc_in_box3d is extract          # the reference's real triangulation test
    host = importlib.import_module("eval_empty_host")
    spec = importlib.util.spec_from_file_location(
        "votenet_config", os.path.join(ROOT, "3dioumatch_amd", "votenet", "config.py"))
    cfgmod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cfgmod)
    cfg = cfgmod.sunrgbd_config()

    class RefConfig(object):
        num_class = cfg.num_class
        class2angle = staticmethod(cfg.class2angle)

        @staticmethod
        def class2size(pred_cls, residual):
            return cfg.mean_size_arr.astype(np.float64)[pred_cls, :] + residual

    ep, size, heading = make_inputs(cfg, host, seed=31)
    out = {"in::" + k: v.numpy() for k, v in ep.items()}
    base = {"dataset_config": RefConfig, "nms_iou": 0.25, "conf_thresh": 0.05}
    corners_all, _ = ap.predictions2corners3d(dict(ep), base)
    out["corners"] = corners_all.astype(np.float32)
    pts = ep["point_clouds"].numpy()[:, :, 0:3]
    counts = np.zeros((B, K), np.int32)
    for i in range(B):
        for j in range(K):
            counts[i, j] = len(extract(pts[i], ap.flip_axis_to_depth(corners_all[i, j]))[0])
    out["counts"] = counts
    closed = host.count_closed_form(ep["point_clouds"].numpy(), ep["center"].numpy(), size, heading)
    assert np.array_equal(closed, counts), "closed form and triangulation disagree on %d boxes" % \
        int((closed != counts).sum())
    empty = counts < 5
    assert (~empty).any(1).all(), "a scene without a non-empty box"
    assert set(HAND) <= set(counts.ravel().tolist()), "the counts miss one of %s" % (HAND,)
    assert counts[0, K - len(HAND):].tolist() == list(HAND)
    share = empty.mean()
    assert 0.02 <= share <= 0.5, "%.1f %% of the boxes are empty" % (100 * share)
    print("empty boxes", int(empty.sum()), "of", B * K, "| smallest face margin %.2e m" %
          host.face_margin(ep["point_clouds"].numpy(), ep["center"].numpy(), size, heading).min())

    #           remove_empty  3-D   cls_nms use_iou old_type per_class
    variants = {"e3d": (True, True, False, False, False, False),
                "e3dcls": (True, True, True, False, False, True),
                "e3dclsiou": (True, True, True, True, False, True),
                "e2d": (True, False, False, False, False, False),
                "p2d": (False, False, False, False, False, False),
                "e2dold": (True, False, False, False, True, False)}
    assert tuple(variants) == host.VARIANTS
    for tag, flags in variants.items():
        config_dict = dict(base, **dict(zip(host.FLAG_NAMES, flags)))
        ep2 = dict(ep)
        batch = ap.parse_predictions(ep2, config_dict)
        out[tag + "_pred_mask"] = np.asarray(ep2["pred_mask"]).astype(np.int32)
        for i, cur in enumerate(batch):  # the list as (class, proposal index, confidence) triples
            key = {corners_all[i, j].tobytes(): j for j in range(K - 1, -1, -1)}
            out["%s_cls_%d" % (tag, i)] = np.array([c for c, _, _ in cur], np.int64)
            out["%s_j_%d" % (tag, i)] = np.array([key[b.tobytes()] for _, b, _ in cur], np.int64)
            out["%s_conf_%d" % (tag, i)] = np.array([s for _, _, s in cur], np.float32)
        out[tag + "_flags"] = np.array(flags, np.int32)
        print(tag, "kept per scene", out[tag + "_pred_mask"].sum(1).tolist(), "list sizes",
              [len(c) for c in batch])
    path = os.path.join(HERE, "eval_parse_empty_ref.npz")
    np.savez_compressed(path, **out)
    size_kb = os.path.getsize(path) / 1024
    print(path, "%.0f KB" % size_kb)
    assert size_kb < 300


if __name__ == "__main__":
    main()
