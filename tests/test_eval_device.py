"""Device-resident AP evaluation (votenet/eval_helper.py: parse_predictions_device,
parse_groundtruths_device, DeviceAPCalculator), host logic: the two kernels are replaced by stand-ins
built from the oracle's box3d_iou matrix (first strict maximum per class, in numpy) and from
eval_det._mark, the NMS by test_eval_helper._oracle_nms.  The goldens are the REFERENCE's
(tests/golden/make_eval_golden.py, make_evaldet_golden.py).  tests/test_eval_device_gpu.py runs the
same checks with the real kernels."""
import importlib

import numpy as np
import pytest
import torch

from conftest import golden, load_pkg


def _mods():
    load_pkg()
    return (importlib.import_module("3dioumatch_amd.votenet"),
            importlib.import_module("3dioumatch_amd.votenet.eval_det"),
            importlib.import_module("3dioumatch_amd.votenet.eval_helper"))


def standin_match(oracle):
    """eval_helper._eval_match from the oracle's per-scene IoU matrix."""
    def fn(det, keep, det_cls, gt, gt_valid, gt_cls, num_class):
        d, kp, dc = det.cpu().numpy(), keep.cpu().numpy(), det_cls.cpu().numpy()
        g, gv, gc = gt.cpu().numpy(), gt_valid.cpu().numpy(), gt_cls.cpu().numpy()
        (b, k), n_gt, cm = kp.shape, gv.shape[1], max(num_class, 1)
        ovmax = np.full((b, k, cm), -np.inf)
        jmax = np.full((b, k, cm), -1, np.int32)
        for i in range(b):
            if n_gt == 0 or not kp[i].any():
                continue
            iou = oracle.box3d_iou_matrix(d[i], g[i])
            for j in np.nonzero(kp[i])[0]:
                for s in range(cm):
                    c = s if num_class else dc[i, j]
                    for col in np.nonzero(gv[i] & (gc[i] == c))[0]:
                        if iou[j, col] > ovmax[i, j, s]:      # strict: the first maximum, never a NaN
                            ovmax[i, j, s], jmax[i, j, s] = iou[j, col], col
        return torch.from_numpy(ovmax).to(det.device), torch.from_numpy(jmax).to(det.device)
    return fn


def standin_mark(D):
    """eval_helper._eval_mark from eval_det._mark, one call per (class, threshold)."""
    def fn(seg, ovmax, gt_id, npos, thresholds, num_gt, curves):
        seg_h, ov, gid = seg.cpu().numpy(), ovmax.cpu().numpy(), gt_id.cpu().numpy().astype(np.int64)
        npos_h, thr = npos.cpu().numpy(), thresholds.cpu().numpy()
        nt, nc, n = len(thr), len(npos_h), len(ov)
        ap, last = np.zeros((nt, nc)), np.zeros((nt, nc))
        rec, prec = np.zeros((nt, n)), np.zeros((nt, n))
        for t in range(nt):
            for c in range(nc):
                s0, s1 = int(seg_h[c]), int(seg_h[c + 1])
                if s1 == s0:
                    continue
                with np.errstate(invalid="ignore", divide="ignore"):
                    r, p, a = D._mark(-np.arange(s1 - s0, dtype=np.float64), ov[s0:s1], gid[s0:s1],
                                      int(npos_h[c]), float(thr[t]), False)
                rec[t, s0:s1], prec[t, s0:s1], ap[t, c], last[t, c] = r, p, a, r[-1]
        dev = ovmax.device
        out = [torch.from_numpy(x).to(dev) for x in (ap, last)]
        return out + ([torch.from_numpy(x).to(dev) for x in (rec, prec)] if curves else [None, None])
    return fn


@pytest.mark.parametrize("tag", ["scannet", "sunrgbd", "nocls"])
def test_parse_predictions_device_matches_reference(tag, oracle, monkeypatch):
    """The (class, proposal, confidence) lists rebuilt from keep / score / cls are the reference's."""
    V, _, E = _mods()
    from test_eval_helper import _oracle_nms
    monkeypatch.setattr(E, "_nms3d", _oracle_nms(oracle))
    g = golden("eval_parse_ref.npz")
    cfg = V.sunrgbd_config() if tag == "sunrgbd" else V.scannet_config()
    cls_nms, use_iou = (bool(v) for v in g[tag + "_flags"])
    ep = {k.split("::", 1)[1]: torch.from_numpy(g[k]) for k in g.files if k.startswith(tag + "_in::")}
    config_dict = {"dataset_config": cfg, "remove_empty_box": False, "use_3d_nms": True,
                   "nms_iou": 0.25, "use_old_type_nms": False, "cls_nms": cls_nms,
                   "use_iou_for_nms": use_iou, "per_class_proposal": cls_nms, "conf_thresh": 0.05}
    keys_before = set(ep)
    out = E.parse_predictions_device(ep, config_dict)
    assert set(ep) == keys_before                     # the device form leaves the end points alone
    assert set(out) == {"corners", "pred_mask", "keep", "cls", "score"}
    b, k = g[tag + "_pred_mask"].shape
    assert out["corners"].dtype == torch.float32 and tuple(out["corners"].shape) == (b, k, 8, 3)
    assert out["pred_mask"].dtype == torch.bool and out["keep"].dtype == torch.bool
    assert out["cls"].dtype == torch.int64 and out["score"].dtype == torch.float32
    assert tuple(out["score"].shape) == ((b, k, cfg.num_class) if cls_nms else (b, k))
    np.testing.assert_array_equal(out["pred_mask"].numpy().astype(np.int32), g[tag + "_pred_mask"])
    np.testing.assert_allclose(out["corners"].numpy(), g[tag + "_corners"], rtol=0, atol=2e-6)
    keep, score, cls = out["keep"].numpy(), out["score"].numpy(), out["cls"].numpy()
    for i in range(b):
        js = np.nonzero(keep[i])[0]
        if cls_nms:
            got = [(c, j, score[i, j, c]) for c in range(cfg.num_class) for j in js]
        else:
            got = [(int(cls[i, j]), j, score[i, j]) for j in js]
        want_cls, want_j, want_conf = (g["%s_%s_%d" % (tag, n, i)] for n in ("cls", "j", "conf"))
        assert [c for c, _, _ in got] == want_cls.tolist()
        assert [j for _, j, _ in got] == want_j.tolist()
        assert np.abs(np.array([s for _, _, s in got], np.float64) - want_conf).max(initial=0) <= 2e-6


def golden_batches(g, dev, sizes=(5, 5, 6), k=17, n_gt=7):
    """The 16 scans of evaldet_ref.npz as (pred, gt) device dicts in single-class mode, padded to k
    proposals and n_gt ground-truth slots, in steps of `sizes` scans."""
    out, scan = [], 0
    for b in sizes:
        corners, keep = np.zeros((b, k, 8, 3), np.float32), np.zeros((b, k), bool)
        cls, score = np.zeros((b, k), np.int64), np.zeros((b, k), np.float32)
        gbox, valid, gcls = np.zeros((b, n_gt, 8, 3), np.float32), np.zeros((b, n_gt), bool), np.zeros((b, n_gt), np.int64)
        for i in range(b):
            n = len(g["det_%d_cls" % scan])
            assert g["det_%d_score" % scan].dtype == np.float32 and n <= k
            corners[i, :n], keep[i, :n] = g["det_%d_box" % scan], True
            cls[i, :n], score[i, :n] = g["det_%d_cls" % scan], g["det_%d_score" % scan]
            m = len(g["gt_%d_cls" % scan])
            assert m <= n_gt
            if m:
                gbox[i, :m], gcls[i, :m] = g["gt_%d_box" % scan], g["gt_%d_cls" % scan]
            valid[i, :m] = True
            scan += 1
        t = lambda *arrays: [torch.from_numpy(a).to(dev) for a in arrays]  # noqa: E731
        out.append((dict(zip(("corners", "keep", "cls", "score"), t(corners, keep, cls, score))),
                    dict(zip(("corners", "valid", "cls"), t(gbox, valid, gcls)))))
    assert scan == int(g["num_scans"])
    return out


def check_golden_ap(E, dev):
    """One DeviceAPCalculator for both thresholds against the reference's rec / prec / ap / metrics."""
    g = golden("evaldet_ref.npz")
    calc = E.DeviceAPCalculator((0.25, 0.5), None)
    for pred, gt in golden_batches(g, dev):
        calc.step(pred, gt)
    assert calc.scan_cnt == 16
    results, metrics = calc.eval_det(), calc.compute_metrics()
    assert len(results) == len(metrics) == 2
    for thr, (rec, prec, ap), met in zip((0.25, 0.5), results, metrics):
        classes = sorted(int(k.split("_")[-1]) for k in g.files if k.startswith("ap_%g_" % thr))
        assert sorted(ap.keys()) == classes
        for c in classes:
            np.testing.assert_allclose(rec[c], g["rec_%g_%d" % (thr, c)], rtol=0, atol=1e-12)
            np.testing.assert_allclose(prec[c], g["prec_%g_%d" % (thr, c)], rtol=0, atol=1e-12)
            assert ap[c] == pytest.approx(float(g["ap_%g_%d" % (thr, c)]), abs=1e-12)
        keys = sorted(met.keys())
        assert keys == [str(k) for k in g["metrics_%g_keys" % thr]]
        np.testing.assert_allclose([met[k] for k in keys], g["metrics_%g_vals" % thr], rtol=0, atol=1e-12)
    calc.reset()
    assert calc.scan_cnt == 0 and calc.eval_det() == [({}, {}, {}), ({}, {}, {})]


def test_device_ap_calculator_matches_reference_hostlogic(oracle, monkeypatch):
    _, D, E = _mods()
    monkeypatch.setattr(E, "_eval_match", standin_match(oracle))
    monkeypatch.setattr(E, "_eval_mark", standin_mark(D))
    check_golden_ap(E, torch.device("cpu"))


def test_device_ap_class_semantics_hostlogic(oracle, monkeypatch):
    """A class with ground truth and no detection reports 0 / 0 / 0, one with detections and no ground
    truth NaN, a class with neither is not reported; equal scores keep (scan, proposal) order."""
    _, D, E = _mods()
    monkeypatch.setattr(E, "_eval_match", standin_match(oracle))
    monkeypatch.setattr(E, "_eval_mark", standin_mark(D))
    a = golden("evaldet_ref.npz")["pair_a"]
    shifted = a[3] + np.float32(0.01)
    # scan 0: two equal-score detections of a[3] (class 0): the first is the TP; one detection of class 2
    # (no ground truth of class 2 anywhere); ground truth: a[3] class 0, a[5] class 4 (never detected)
    pred = {"corners": torch.from_numpy(np.stack([shifted, a[3] + np.float32(0.02), a[7]])[None]),
            "keep": torch.ones(1, 3, dtype=torch.bool), "cls": torch.tensor([[0, 0, 2]]),
            "score": torch.tensor([[0.5, 0.5, 0.9]])}
    gt = {"corners": torch.from_numpy(np.stack([a[3], a[5]])[None]),
          "valid": torch.ones(1, 2, dtype=torch.bool), "cls": torch.tensor([[0, 4]])}
    calc = E.DeviceAPCalculator((0.5,), {0: "zero", 2: "two", 4: "four"})
    calc.step(pred, gt)
    (rec, prec, ap), = calc.eval_det()
    assert sorted(ap) == [0, 2, 4]
    np.testing.assert_allclose(rec[0], [1.0, 1.0])
    np.testing.assert_allclose(prec[0], [1.0, 0.5])
    assert ap[0] == pytest.approx(1.0)
    assert ap[4] == 0 and rec[4] == 0 and prec[4] == 0
    assert np.isnan(ap[2]) and np.isnan(rec[2]).all()
    with np.errstate(invalid="ignore"):
        met, = calc.compute_metrics()
    assert list(met) == ["zero Average Precision", "two Average Precision", "four Average Precision", "mAP",
                         "zero Recall", "two Recall", "four Recall", "AR"]
    assert met["zero Recall"] == 1.0 and met["four Recall"] == 0 and np.isnan(met["two Recall"])
    # the host path on the same scan
    host = E.APCalculator(0.5, {0: "zero", 2: "two", 4: "four"})
    monkeypatch.setattr(D, "_best_match", lambda det, b, c, g, device: oracle.best_match(det, b, c, g))
    host.step([[(0, shifted, 0.5), (0, a[3] + np.float32(0.02), 0.5), (2, a[7], 0.9)]], [[(0, a[3]), (4, a[5])]])
    with np.errstate(invalid="ignore", divide="ignore"):
        want = host.compute_metrics()
    assert set(want) == set(met)
    np.testing.assert_allclose([met[k] for k in want], [want[k] for k in want], rtol=0, atol=1e-12, equal_nan=True)


def test_device_ap_rejects_class_ids_beyond_the_bins(oracle, monkeypatch):
    _, D, E = _mods()
    monkeypatch.setattr(E, "_eval_match", standin_match(oracle))
    monkeypatch.setattr(E, "_eval_mark", standin_mark(D))
    a = golden("evaldet_ref.npz")["pair_a"]
    pred = {"corners": torch.from_numpy(a[None, :2]), "keep": torch.ones(1, 2, dtype=torch.bool),
            "cls": torch.tensor([[0, 64]]), "score": torch.tensor([[0.5, 0.4]])}
    gt = {"corners": torch.from_numpy(a[None, :1]), "valid": torch.ones(1, 1, dtype=torch.bool),
          "cls": torch.tensor([[0]])}
    calc = E.DeviceAPCalculator()
    calc.step(pred, gt)
    with pytest.raises(ValueError, match="class ids"):
        calc.compute_metrics()


def test_device_ap_has_no_cpu_path():
    _, D, E = _mods()
    g = golden("evaldet_ref.npz")
    pred, gt = golden_batches(g, torch.device("cpu"))[0]
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.DeviceAPCalculator().step(pred, gt)
    with pytest.raises(RuntimeError, match="no CPU path"):
        D.eval_mark_gpu(torch.zeros(2, dtype=torch.int64), torch.zeros(0, dtype=torch.float64),
                        torch.zeros(0, dtype=torch.int32), torch.zeros(1, dtype=torch.int64),
                        torch.zeros(1, dtype=torch.float64), 0)


def test_eval_entry_points_gate_on_the_host():
    """iou3d_eval_match / iou3d_eval_mark return an error code outside their gates before anything is
    launched (no device needed)."""
    import ctypes
    _, D, _ = _mods()
    lib = importlib.import_module("3dioumatch_amd._lib").lib
    for b, k, g, c in ((1, 0, 4, 0), (1, 4, -1, 0), (1, 4, 4, 65), (1, 4, 4, -1), (-1, 4, 4, 0)):
        a = D.EvalMatchArgs()
        a.B, a.K, a.G, a.C = b, k, g, c
        assert lib.iou3d_eval_match(ctypes.byref(a), None) != 0, (b, k, g, c)
    a = D.EvalMatchArgs()
    a.B, a.K, a.G, a.C = 0, 4, 4, 0                    # no scene: nothing to do
    assert lib.iou3d_eval_match(ctypes.byref(a), None) == 0
    for n, nc, nt in ((-1, 4, 1), (2 ** 31, 4, 1), (8, 0, 1), (8, 65, 1), (8, 4, 0)):
        m = D.EvalMarkArgs()
        m.n, m.num_class, m.num_thresh, m.num_gt = n, nc, nt, 4
        assert lib.iou3d_eval_mark(ctypes.byref(m), None) != 0, (n, nc, nt)


# ---------------------------------------------------------------------------------------------
# the marking past one 256-detection chunk per class: eval_det._mark (the host path and
# standin_mark above) against the plain loop of tests/eval_mark_cases.py
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", [0.25, 0.5])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_mark_matches_loop_reference(seed, thr):
    import eval_mark_cases as M
    _, D, _ = _mods()
    case, want = M.mark_case(seed), M.reference(seed, thr)
    checked = 0
    for c, length in enumerate(M.LENGTHS):
        if length == 0:
            assert want[c] is None
            continue
        ov, gid, npos = M.segment(case, c)
        with np.errstate(invalid="ignore", divide="ignore"):
            rec, prec, ap = D._mark(-np.arange(length, dtype=np.float64), ov, gid.astype(np.int64), npos, thr, False)
        wrec, wprec, wap = want[c]
        np.testing.assert_array_equal(rec, wrec)        # NaN == NaN here
        np.testing.assert_array_equal(prec, wprec)
        assert (np.isnan(ap) and np.isnan(wap)) or abs(ap - wap) <= 1e-12, (c, ap, wap)
        assert np.isnan(wap) == (npos == 0)
        checked += 1
    assert checked == 9


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_mark_case_builder_keeps_its_edges(seed):
    """What tests/eval_mark_cases.py promises about mark_case, so that an edit cannot empty the case."""
    import eval_mark_cases as M
    case = M.mark_case(seed)
    seg, npos = case["seg"], case["npos"]
    assert tuple(np.diff(seg)) == M.LENGTHS and tuple(npos) == M.NPOS and len(case["ovmax"]) == 5631
    assert case["ovmax"].dtype == np.float64 and case["gt_id"].dtype == np.int32 and seg.dtype == np.int64
    assert case["num_gt"] == sum(M.NPOS) + 5
    base = np.concatenate([[0], np.cumsum(npos)])
    for c, length in enumerate(M.LENGTHS):
        ov, gid, p = M.segment(case, c)
        inf = np.isneginf(ov)
        assert (gid[inf] == 0).all() and not np.isnan(ov).any()
        assert ((gid[~inf] >= base[c]) & (gid[~inf] < base[c] + p)).all()
        assert ((ov[~inf] >= 0) & (ov[~inf] <= 1)).all()
        if length >= 255 and c not in (M.ALL_INF, M.REVERSED):
            assert (ov == 0.25).any() and (ov == 0.5).any() and 0.05 * length < inf.sum() < 0.2 * length
    ov, _, p = M.segment(case, M.ALL_INF)
    assert p == 0 and len(ov) == 300 and np.isneginf(ov).all()
    ov, _, _ = M.segment(case, M.REVERSED)
    assert np.isneginf(ov[:M.REVERSED_FROM]).all() and M.REVERSED_FROM == 3 * M.CHUNK
    for thr in (0.25, 0.5):
        want = M.reference(seed, thr)
        long = [c for c, length in enumerate(M.LENGTHS) if length > M.CHUNK and c != M.ALL_INF]
        assert long == [4, 5, 6, 9, 10]
        assert any(0 < want[c][2] < 1 for c in long)
        assert any(want[c][0][-1] < 1 for c in long)
        assert any(M.cross_chunk_claims(*M.segment(case, c)[:2], thr) >= 5 for c in long)
        assert any(M.raised_chunks(want[c][1]) for c in long)
        # the long score-ordered segments: 0 < AP < 1 in 513, 1000 and 2049, repeat claims across chunks in
        # 1000 and 2049, a raised envelope in 513 and 1000, a final recall below 1 in 513
        for c in (5, 6, 9):
            assert 0 < want[c][2] < 1
        for c in (6, 9):
            assert M.cross_chunk_claims(*M.segment(case, c)[:2], thr) >= 5
        for c in (5, 6):
            assert M.raised_chunks(want[c][1])
        assert want[5][0][-1] < 0.5
        # the reversed segment: true positives only in its last chunk, every earlier chunk raised from it
        rec, prec, ap = want[M.REVERSED]
        assert rec[M.REVERSED_FROM - 1] == 0 and rec[-1] > 0 and ap > 0
        assert M.raised_chunks(prec) == [0, 1, 2]
        assert np.isnan(want[M.ALL_INF][2]) and np.isnan(want[M.ALL_INF][0]).all()
    assert M.permuted_ids(case).dtype == np.int32 and not np.array_equal(M.permuted_ids(case), case["gt_id"])


def test_mark_envelope_from_a_distant_chunk():
    """eval_mark_cases.envelope_case: the case is what it says, and _mark agrees with the loop on it."""
    import eval_mark_cases as M
    _, D, _ = _mods()
    case = M.envelope_case()
    ov, gid, npos = M.segment(case, 0)
    wrec, wprec, wap = M.loop_mark(ov, gid, npos, 0.5)
    assert len(ov) == 3 * M.CHUNK + 5 and M.raised_chunks(wprec) == [0, 1, 2]
    assert wprec.argmax() == len(ov) - 1 and wprec[-1] == 278 / 773 and wprec[:-1].max() < wprec[-1]
    assert wrec[M.CHUNK - 1] == 16 / 300 and wrec[-1] == 278 / 300
    # the AP with the envelope of the next chunk only, or of the chunks up to the third, is another number
    assert abs(wap - (278 / 300) * (278 / 773)) < 0.05 * wap
    rec, prec, ap = D._mark(-np.arange(len(ov), dtype=np.float64), ov, gid.astype(np.int64), npos, 0.5, False)
    np.testing.assert_array_equal(rec, wrec)
    np.testing.assert_array_equal(prec, wprec)
    assert abs(ap - wap) <= 1e-12
