"""Device-resident AP evaluation on the MI355X: the match kernel (csrc/eval_ap.hip) against the
oracle stand-in, also at K, G and C off its 4 x 64 tile; the marking kernel directly against the plain
loop of tests/eval_mark_cases.py on class segments of up to 9 chunks of 256 detections; the reference's
golden AP with both kernels; parity of DeviceAPCalculator with the host path (APCalculator / eval_det)
on end points with shifted and duplicated true boxes, over one and two steps; the absence of host
synchronisation in the per-batch calls, and evaluate(..., device_ap=True) of both evaluation loops
against device_ap=False."""
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


def _match_case(rng, b=3, k=40, g=70, bases=17, classes=CLASSES, absent=3, offsets=(0.0, 0.03, 0.06, 0.09)):
    """Boxes of _random_corners(spread 1.5).  Independent random boxes would leave about 55 of the 600
    slots above IoU 0.25 (measured with the oracle), so a scene is built from `bases` random boxes:
    ground-truth slot j < len(offsets) * bases is base box j % bases moved by offsets[j // bases] along x
    (3 cm per copy by default), its copies in consecutive classes of `classes`; proposal i is base box
    i % bases moved by 1 cm + 2 mm * i along z.  With the defaults every kept proposal then has a box
    above 0.25 in each class present, and the columns of a class lie on both sides of the 64-column
    tile.  The other slots are random boxes of random classes.  Where g - 2 >= 64, slot g - 2 repeats
    the early slot min(3, g - 1) with its class (the first index must win, across the tile boundary);
    slot g - 1 is a free box; about 5 % of the slots are invalid, the last of several scenes has no
    valid slot, a quarter of the proposals is not kept.  A proposal's class is one of `classes` or
    `absent`.  g = 65 or 129: the free box is alone in the last tile, so the last proposal is put on it
    (kept, with its class): that tile wins somewhere."""
    det = np.zeros((b, k, 8, 3), np.float32)
    gt = np.zeros((b, g, 8, 3), np.float32)
    gt_cls = np.zeros((b, g), np.int64)
    built = min(len(offsets) * bases, g)
    early, rep = min(3, g - 1), (g - 2 if g - 2 >= 64 else None)
    for s in range(b):
        base = _random_corners(rng, bases, 1.5)
        for i in range(k):
            det[s, i] = base[i % bases] + np.array([0, 0, 0.01 + 0.002 * i], np.float32)
        for j in range(built):
            gt[s, j] = base[j % bases] + np.array([offsets[j // bases], 0, 0], np.float32)
            gt_cls[s, j] = classes[(j // bases + j % bases) % len(classes)]
        if g > built:
            gt[s, built:] = _random_corners(rng, g - built, 1.5)
            gt_cls[s, built:] = rng.choice(classes, g - built)
        if rep is not None:
            gt[s, rep], gt_cls[s, rep] = gt[s, early], gt_cls[s, early]
    keep = rng.random((b, k)) > 0.25
    valid = rng.random((b, g)) > 0.05
    valid[:, [early] + ([] if rep is None else [rep])] = True
    if b > 1:
        valid[b - 1] = False
    det_cls = rng.choice(tuple(classes) + (() if absent is None else (absent,)), (b, k))
    first = min(3, k - 1)
    keep[:, first], det_cls[:, first] = True, gt_cls[:, early]      # proposal 3 competes for the repeated box
    if g > 64 and g % 64 == 1:
        det[:, k - 1] = gt[:, g - 1] + np.array([0, 0, 0.01], np.float32)
        keep[:, k - 1], det_cls[:, k - 1] = True, gt_cls[:, g - 1]
        valid[:b - 1 if b > 1 else b, g - 1] = True
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


def _cls_except(c, absent):
    return tuple(i for i in range(c) if i != absent)


# (B, K, G, C) -> the builder's arguments, tuned with the oracle alone until at least a quarter of the
# (kept proposal, present class) slots lies above IoU 0.25: few bases, so that a base has a copy in most
# classes, and copy offsets of millimetres.  Where the offsets do not grow with the copy, the best copy of
# a class sits in a later tile than its first, and a best carried from the first tile must survive.
RAGGED = {
    # one lane of one tile, one slot
    (1, 1, 1, 1): dict(bases=1, classes=(0,), absent=None, offsets=(0.0,)),
    # exactly one tile; K = 5: a row tile with one live row; the workload's class count
    (2, 5, 64, 18): dict(bases=5, classes=_cls_except(18, 7), absent=7, offsets=tuple(0.01 * m for m in range(12))),
    # one column in the second tile; three live rows in the last row tile
    (2, 43, 65, 18): dict(bases=4, classes=_cls_except(18, 7), absent=7, offsets=tuple(0.01 * m for m in range(16))),
    # one column in the third tile; C = 64: all 256 lanes are slots; the best copy is copy 45 (second tile)
    (1, 41, 129, 64): dict(bases=2, classes=_cls_except(64, 21), absent=21,
                           offsets=tuple(0.003 * abs(m - 45) for m in range(63))),
    # four tiles, single-class mode; the best copy of three classes in four is copy 19 .. 21 (third tile),
    # of the fourth copy 2 (first tile)
    (3, 7, 200, 0): dict(bases=7, classes=CLASSES, absent=3,
                         offsets=tuple(0.01 * min(abs(m - 2) + 1, abs(m - 20)) for m in range(28))),
    # one class: every column is every slot's
    (2, 43, 129, 1): dict(bases=43, classes=(0,), absent=None, offsets=(0.0, 0.03)),
}


def _slots_that_count(arrays, num_class):
    """(kept proposal, present class) slots as a mask of the (B, K, max(C, 1)) outputs; a class is present
    in a scene where a valid ground-truth box has it"""
    _, keep, det_cls, _, valid, gt_cls = arrays
    b, k = keep.shape
    present = np.zeros((b, 65), bool)
    for s in range(b):
        present[s, gt_cls[s][valid[s]]] = True
    if num_class:
        return keep[:, :, None] & present[:, None, :num_class]
    return (keep & np.take_along_axis(present, det_cls, 1))[:, :, None]


@pytest.mark.parametrize("shape", list(RAGGED), ids=lambda s: "B%d-K%d-G%d-C%d" % s)
def test_match_kernel_ragged_shapes(shape, oracle):
    """K off the 4-row tile, G at 1, 64, 65, 129 and 200 columns, C at 1, 18, 64 and single-class mode."""
    _, D, _ = _mods()
    b, k, g, num_class = shape
    arrays = _match_case(np.random.default_rng(13), b, k, g, **RAGGED[shape])
    ov, jm = D.eval_match_gpu(*[torch.from_numpy(a).to(DEV) for a in arrays], num_class)
    wov, wjm = standin_match(oracle)(*[torch.from_numpy(a) for a in arrays], num_class)
    ov, jm, wov, wjm = ov.cpu().numpy(), jm.cpu().numpy(), wov.numpy(), wjm.numpy()
    keep, valid = arrays[1], arrays[4]
    assert ov.shape == wov.shape == (b, k, max(num_class, 1)) and jm.dtype == np.int32
    # the oracle's answer is not mostly -inf
    count = _slots_that_count(arrays, num_class)
    above = (wov[count] > 0.25).mean()
    print("slots above 0.25: %d of %d" % ((wov[count] > 0.25).sum(), count.sum()))
    assert count.sum() >= 1 and above >= 0.25, above
    if shape == (1, 1, 1, 1):
        assert wov[0, 0, 0] > 0.25
    np.testing.assert_array_equal(jm, wjm)
    assert np.array_equal(np.isneginf(ov), np.isneginf(wov)) and not np.isnan(ov).any()
    fin = np.isfinite(wov)
    np.testing.assert_allclose(ov[fin], wov[fin], rtol=0, atol=1e-13)
    # the ragged last row tile
    tail = slice(k - k % 4, k)
    assert k % 4 and keep[:, tail][valid.any(1)].any() and (wjm[:, tail] >= 0).any()
    np.testing.assert_array_equal(jm[:, tail], wjm[:, tail])
    np.testing.assert_allclose(ov[:, tail][fin[:, tail]], wov[:, tail][fin[:, tail]], rtol=0, atol=1e-13)
    assert np.isneginf(ov[~keep]).all() and (jm[~keep] == -1).all()              # not kept
    if b > 1:
        assert np.isneginf(ov[b - 1]).all() and (jm[b - 1] == -1).all()          # no valid ground truth
    if g - 2 >= 64:
        assert not (jm == g - 2).any()                                           # the second of two equal boxes
    if g > 128:
        assert (jm >= 128).any() and ((jm >= 0) & (jm < 64)).any()               # the third tile, the first
    if g > 64 and g % 64 == 1:
        assert (jm == g - 1).any() and ((jm >= 0) & (jm < 64)).any()             # the last tile's only column
    if RAGGED[shape]["absent"] is not None and num_class:
        absent = RAGGED[shape]["absent"]
        assert np.isneginf(ov[:, :, absent]).all() and (jm[:, :, absent] == -1).all()


def _bits(t):
    return t.contiguous().view(torch.int64)


@pytest.mark.parametrize("pad", [False, True], ids=["11-classes", "64-classes"])
@pytest.mark.parametrize("thresholds", [(0.25, 0.5), (0.5,), (0.1, 0.25, 0.5)], ids=lambda t: "thr" + "-".join(map(str, t)))
@pytest.mark.parametrize("seed", [0, 1])
def test_mark_kernel_matches_loop_reference(seed, thresholds, pad):
    """eval_mark_gpu directly, on class segments of 0 .. 2049 detections (up to 9 chunks of 256), against
    tests/eval_mark_cases.loop_mark.  rec and prec are each ONE float64 division of two integers (the
    library is built without contraction or fast-math), so they are compared exactly; AP and the last
    recall differ from the reference only in the order of a sum of at most 2049 terms of at most 1."""
    import eval_mark_cases as M
    _, D, _ = _mods()
    case = M.mark_case(seed)
    seg, npos, n = case["seg"], case["npos"], len(case["ovmax"])
    nc = len(M.LENGTHS)
    if pad:     # the grid the calculator launches: 64 classes, the others without detections
        seg = np.concatenate([seg, np.full(64 - nc, seg[-1])])
        npos = np.concatenate([npos, np.zeros(64 - nc, np.int64)])
    # 7 entries after the last segment (the calculator's slots that are no detection): never read, never written
    extra = 7
    ovmax = np.concatenate([case["ovmax"], np.full(extra, 0.9)])
    own = int(np.cumsum(M.NPOS)[8])        # an id of the class of 2049
    dev = lambda a: torch.tensor(np.asarray(a), device=DEV)  # noqa: E731
    thr = torch.tensor(thresholds, dtype=torch.float64, device=DEV)

    def run(gt_id, curves):
        gid = np.concatenate([gt_id, np.full(extra, own, np.int32)])
        return D.eval_mark_gpu(dev(seg), dev(ovmax), dev(gid), dev(npos), thr, case["num_gt"], curves=curves)

    ap_d, last_d, rec_d, prec_d = run(case["gt_id"], True)
    ap, last, rec, prec = (x.cpu().numpy() for x in (ap_d, last_d, rec_d, prec_d))
    assert ap.shape == last.shape == (len(thresholds), len(npos)) and rec.shape == prec.shape == (len(thresholds), n + extra)
    worst_curve = worst_ap = 0.0
    for t, th in enumerate(thresholds):
        want = M.reference(seed, th)
        for c in range(nc):
            s0, s1 = int(seg[c]), int(seg[c + 1])
            if want[c] is None:
                continue
            wrec, wprec, wap = want[c]
            for got, w in ((rec[t, s0:s1], wrec), (prec[t, s0:s1], wprec)):
                assert np.array_equal(np.isnan(got), np.isnan(w))
                worst_curve = max(worst_curve, np.abs(got - w)[~np.isnan(w)].max(initial=0.0))
            if not np.isnan(wap):
                worst_ap = max(worst_ap, abs(ap[t, c] - wap), abs(last[t, c] - wrec[-1]))
    print("largest rec / prec difference %.3e, largest AP / last-recall difference %.3e" % (worst_curve, worst_ap))
    for t, th in enumerate(thresholds):
        want = M.reference(seed, th)
        for c in range(len(npos)):
            s0, s1 = int(seg[c]), int(seg[c + 1])
            if c >= nc or want[c] is None:
                assert s1 == s0 and ap[t, c] == 0 and last[t, c] == 0, (th, c)
                continue
            wrec, wprec, wap = want[c]
            np.testing.assert_array_equal(rec[t, s0:s1], wrec, err_msg="rec thr %g class %d" % (th, c))
            np.testing.assert_array_equal(prec[t, s0:s1], wprec, err_msg="prec thr %g class %d" % (th, c))
            np.testing.assert_allclose(ap[t, c], wap, rtol=0, atol=1e-12, equal_nan=True)
            np.testing.assert_allclose(last[t, c], wrec[-1], rtol=0, atol=1e-12, equal_nan=True)
            assert np.isnan(wap) == np.isnan(ap[t, c]) == np.isnan(last[t, c]) == (c == M.ALL_INF)
    assert (rec[:, n:] == 0).all() and (prec[:, n:] == 0).all()                 # outside every segment

    ap2, last2, rec2, prec2 = run(case["gt_id"], False)
    assert rec2 is None and prec2 is None
    assert torch.equal(_bits(ap2), _bits(ap_d)) and torch.equal(_bits(last2), _bits(last_d))

    # the claim may depend only on WHICH detections share an id
    ap3, last3, rec3, prec3 = run(M.permuted_ids(case), True)
    for a, b in ((ap3, ap_d), (last3, last_d), (rec3, rec_d), (prec3, prec_d)):
        assert torch.equal(_bits(a), _bits(b))


def test_mark_kernel_envelope_from_a_distant_chunk():
    """eval_mark_cases.envelope_case: the terms of the first chunk are multiplied by a precision that is
    reached only in the fourth chunk."""
    import eval_mark_cases as M
    _, D, _ = _mods()
    case = M.envelope_case()
    wrec, wprec, wap = M.loop_mark(*M.segment(case, 0), 0.5)
    dev = lambda a: torch.tensor(np.asarray(a), device=DEV)  # noqa: E731
    ap, last, rec, prec = D.eval_mark_gpu(dev(case["seg"]), dev(case["ovmax"]), dev(case["gt_id"]), dev(case["npos"]),
                                          torch.tensor([0.5], dtype=torch.float64, device=DEV), case["num_gt"], curves=True)
    print("AP difference %.3e" % abs(float(ap[0, 0]) - wap))
    np.testing.assert_array_equal(rec[0].cpu().numpy(), wrec)
    np.testing.assert_array_equal(prec[0].cpu().numpy(), wprec)
    np.testing.assert_allclose(float(ap[0, 0]), wap, rtol=0, atol=1e-12)
    np.testing.assert_allclose(float(last[0, 0]), wrec[-1], rtol=0, atol=1e-12)


def test_device_ap_calculator_matches_reference_gpu():
    _, _, E = _mods()
    check_golden_ap(E, DEV)


def _imperfect_end_points(V, cfg, rng, scenes=3):
    """test_eval_det._perfect_end_points with every second true box moved by 0.3 x its size and every
    true box repeated (4 mm off, so that the NMS at 0.999 keeps both) with the same logits."""
    ep = _perfect_end_points(V, cfg, rng, scenes=scenes, k=48)
    mean = torch.from_numpy(cfg.mean_size_arr.astype(np.float32))
    for b in range(scenes):
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


@pytest.mark.parametrize("steps", [1, 2], ids=["one-step", "two-steps"])
@pytest.mark.parametrize("per_class", [True, False], ids=["per-class", "single-class"])
@pytest.mark.parametrize("tag", ["scannet", "sunrgbd"])
def test_device_ap_matches_host_path(tag, per_class, steps):
    """Two steps: the second batch's ground-truth ids start after the first's, the repeated logits tie
    scores across the steps, and with per_class_proposal every class has more than 256 detections (the
    marking kernel's chunk).  The clutter falls to conf_thresh -- about 9 detections a scene are left --
    so the second step has 36 scenes."""
    V, _, E = _mods()
    cfg = V.sunrgbd_config() if tag == "sunrgbd" else V.scannet_config()
    config_dict = {"dataset_config": cfg, "remove_empty_box": False, "use_3d_nms": True,
                   "nms_iou": 0.999, "use_old_type_nms": False, "cls_nms": True,
                   "use_iou_for_nms": False, "per_class_proposal": per_class, "conf_thresh": 0.05}
    dev = E.DeviceAPCalculator((0.25, 0.5), None)
    hosts = [E.APCalculator(thr, None, device="cuda:0") for thr in (0.25, 0.5)]
    preds = []
    for seed, scenes in ((3, 3), (4, 36))[:steps]:
        ep = {k: (v.to(DEV) if torch.is_tensor(v) else v)
              for k, v in _imperfect_end_points(V, cfg, np.random.default_rng(seed), scenes).items()}
        dev.step(E.parse_predictions_device(ep, config_dict), E.parse_groundtruths_device(ep, config_dict))
        batch, gts = E.parse_predictions(ep, config_dict), E.parse_groundtruths(ep, config_dict)
        for host in hosts:
            host.step(batch, gts)
        preds += batch
    assert dev.scan_cnt == hosts[0].scan_cnt == len(preds)
    got = dev.compute_metrics()
    partial = tied = False
    for host, g in zip(hosts, got):
        with np.errstate(invalid="ignore", divide="ignore"):
            want = host.compute_metrics()
        assert list(g) == list(want)
        np.testing.assert_allclose([g[k] for k in want], [want[k] for k in want], rtol=0, atol=1e-12,
                                   equal_nan=True)
        partial |= any(0 < v < 1 for k, v in want.items() if k.endswith("Average Precision"))
    longest = 0
    for c in range(cfg.num_class):
        scores = [s for scan in preds for cc, _, s in scan if cc == c]
        tied |= len(set(scores)) < len(scores)
        longest = max(longest, len(scores))
    assert partial and tied      # ordering and first-claim were exercised
    print("detections of the longest class:", longest)
    if per_class and steps == 2:
        assert longest > 256, longest


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
