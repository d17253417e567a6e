"""Host implementations the remove_empty_box / 2-D NMS tests compare against (test_eval_empty.py,
test_eval_empty_gpu.py) -- numpy restatements of the formulas, independent of the kernels:

  count_closed_form   the point-in-oriented-box test of include/lhs_hip.h (lhs_box_point_count): box
                      frame in float64 rounded to float32, per-pair arithmetic in float32
  face_margin         distance of every (point, box) pair to the box's surface, in float64
  camera_aabb         axis-aligned camera-frame bounds of get_3d_box (float32 corners)
  nms_masked          the greedy loop of utils/nms.py (nms_2d_faster / nms_3d_faster /
                      nms_3d_faster_samecls) on the valid subset, ties of the ascending sort by index
"""
import numpy as np

VARIANTS = ("e3d", "e3dcls", "e3dclsiou", "e2d", "p2d", "e2dold")
FLAG_NAMES = ("remove_empty_box", "use_3d_nms", "cls_nms", "use_iou_for_nms", "use_old_type_nms",
              "per_class_proposal")


def _frame(center, size, heading):
    c = np.cos(heading.astype(np.float64)).astype(np.float32)
    s = np.sin(heading.astype(np.float64)).astype(np.float32)
    half = (size.astype(np.float64) / 2).astype(np.float32)
    return c, s, center.astype(np.float32), half


def count_closed_form(points, center, size, heading):
    """points (S,N,>=3) f32, center (S,n,3) f32, size (S,n,3) f64, heading (S,n) f64 -> (S,n) i32"""
    c, s, ctr, half = _frame(center, size, heading)
    out = np.zeros(heading.shape, np.int32)
    for i in range(heading.shape[0]):
        p = points[i, :, :3].astype(np.float32)
        d = p[None, :, :] - ctr[i][:, None, :]                                     # (n,N,3) f32
        xr = c[i][:, None] * d[..., 0] - s[i][:, None] * d[..., 1]
        zr = s[i][:, None] * d[..., 0] + c[i][:, None] * d[..., 1]
        assert xr.dtype == np.float32 and zr.dtype == np.float32
        inside = (np.abs(xr) <= half[i][:, None, 0]) & (np.abs(zr) <= half[i][:, None, 1]) & \
            (np.abs(d[..., 2]) <= half[i][:, None, 2])
        out[i] = inside.sum(1)
    return out


def face_margin(points, center, size, heading):
    """(S,n,N) f64: how far each point is from the surface of each box (Chebyshev-style: the
    smallest |coordinate| - half extent gap among the faces the point could cross); float64."""
    out = []
    for i in range(heading.shape[0]):
        c, s = np.cos(heading[i].astype(np.float64)), np.sin(heading[i].astype(np.float64))
        d = points[i, None, :, :3].astype(np.float64) - center[i][:, None, :].astype(np.float64)
        xr = c[:, None] * d[..., 0] - s[:, None] * d[..., 1]
        zr = s[:, None] * d[..., 0] + c[:, None] * d[..., 1]
        gap = np.stack([np.abs(xr), np.abs(zr), np.abs(d[..., 2])], -1) - \
            (size[i].astype(np.float64) / 2)[:, None, :]                           # < 0 inside
        # outside: the largest positive gap bounds the distance from below; inside: the smallest |gap|
        out.append(np.where((gap <= 0).all(-1), np.abs(gap).min(-1), gap.max(-1)))
    return np.stack(out)


def camera_aabb(center, size, heading):
    """(n,3) f32, (n,3) f64, (n,) f64 -> (n,6) f32 (x1,y1,z1,x2,y2,z2) of the float32 corners of
    get_3d_box on the camera-frame centre (the arithmetic of votenet/eval_helper.py)."""
    sx = np.array([1, 1, -1, -1, 1, 1, -1, -1], np.float64)
    sy = np.array([1, 1, 1, 1, -1, -1, -1, -1], np.float64)
    sz = np.array([1, -1, -1, 1, 1, -1, -1, 1], np.float64)
    size = size.astype(np.float64)
    x, y, z = sx * size[:, 0:1] / 2, sy * size[:, 2:3] / 2, sz * size[:, 1:2] / 2
    c, s = np.cos(heading)[:, None], np.sin(heading)[:, None]
    cx, cy, cz = (center[:, 0:1].astype(np.float64), -center[:, 2:3].astype(np.float64),
                  center[:, 1:2].astype(np.float64))
    px = ((c * x + 0.0 * y + s * z) + cx).astype(np.float32)
    py = ((0.0 * x + 1.0 * y + 0.0 * z) + cy).astype(np.float32)
    pz = ((-s * x + 0.0 * y + c * z) + cz).astype(np.float32)
    return np.stack([px.min(1), py.min(1), pz.min(1), px.max(1), py.max(1), pz.max(1)], 1)


def nms_masked(aabb, score, cls, thresh, old_type, same_class, dims, valid):
    """aabb (n,6) f32, score (n,) f32, cls (n,) i64 or None, valid (n,) or None -> picked (n,) bool"""
    n = len(score)
    b = aabb.astype(np.float64)
    ext = b[:, 3:6] - b[:, 0:3]
    area = ext[:, 0] * ext[:, 2] if dims == 2 else ext[:, 0] * ext[:, 1] * ext[:, 2]
    order = np.lexsort((np.arange(n), score))           # ascending score, ties by index
    if valid is not None:
        order = order[np.asarray(valid)[order] != 0]
    picked = np.zeros(n, bool)
    I = order
    while I.size:
        i, rest = I[-1], I[:-1]
        picked[i] = True
        lo = np.maximum(b[i, 0:3], b[rest, 0:3])
        hi = np.minimum(b[i, 3:6], b[rest, 3:6])
        e = np.maximum(0, hi - lo)
        inter = e[:, 0] * e[:, 2] if dims == 2 else e[:, 0] * e[:, 1] * e[:, 2]
        o = inter / area[rest] if old_type else inter / (area[i] + area[rest] - inter)
        if same_class:
            o = o * (cls[i] == cls[rest])
        I = rest[~(o > thresh)]
    return picked


def nms_masked_batch(center, size, heading, score, cls, thresh, old_type, same_class, dims, valid):
    """numpy (S,...) arrays -> (S,n) bool"""
    return np.stack([
        nms_masked(camera_aabb(center[i], size[i], heading[i]), score[i],
                   None if cls is None else cls[i], thresh, old_type, same_class, dims,
                   None if valid is None else valid[i]) for i in range(score.shape[0])])


# --- the golden of tests/golden/make_eval_empty_golden.py ---

def config_of(V, g, tag):
    """the config_dict of golden variant `tag` (V: the votenet package)"""
    flags = {n: bool(v) for n, v in zip(FLAG_NAMES, g[tag + "_flags"])}
    return dict({"dataset_config": V.sunrgbd_config(), "nms_iou": 0.25, "conf_thresh": 0.05}, **flags)


def inputs_of(g, dev):
    import torch
    return {k.split("::", 1)[1]: torch.from_numpy(g[k]).to(dev) for k in g.files if k.startswith("in::")}


def check_against_golden(g, tag, ep, batch, config_dict):
    assert isinstance(ep["pred_mask"], np.ndarray) and ep["pred_mask"].dtype == np.float64
    np.testing.assert_array_equal(ep["pred_mask"].astype(np.int32), g[tag + "_pred_mask"])
    if config_dict["remove_empty_box"]:
        assert isinstance(ep["nonempty_box_mask"], np.ndarray) and ep["nonempty_box_mask"].dtype == np.float64
        np.testing.assert_array_equal(ep["nonempty_box_mask"], (g["counts"] >= 5).astype(np.float64))
        assert not (ep["pred_mask"] * (1 - ep["nonempty_box_mask"])).any()   # no empty box survives
    else:
        assert "nonempty_box_mask" not in ep
    for i, cur in enumerate(batch):
        want_cls, want_j, want_conf = (g["%s_%s_%d" % (tag, n, i)] for n in ("cls", "j", "conf"))
        assert len(cur) == len(want_cls)
        assert [c for c, _, _ in cur] == want_cls.tolist()
        for (c, box, conf), j, wc in zip(cur, want_j, want_conf):
            assert np.allclose(box, g["corners"][i, j], rtol=0, atol=2e-6)
            assert abs(conf - wc) <= 2e-6
