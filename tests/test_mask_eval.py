"""The mask matching on the host: host_match_masks against a brute force with Python sets, hand-built
cases with known answers (through MaskAPCalculator's host path, whose marker is eval_det._mark),
PointTruth's refusals, the exports and the tool's flags."""
import importlib
import importlib.util
import os

import numpy as np
import pytest

import label_points_cases as cases
import mask_eval_cases as mcases
from conftest import load_pkg

load_pkg()
V = importlib.import_module("3dioumatch_amd.votenet")
ME = importlib.import_module("3dioumatch_amd.votenet.mask_eval")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = ME.NOT_A_DETECTION
_hand = [0]


def hand(owners, ti, tc, cls, score, count=None, cap=None):
    """(labels, found, truth) of one hand-built case on the host; scans are lists of per-point values."""
    cap = cap or len(cls[0])
    pad = lambda rows, fill: [list(r) + [fill] * (cap - len(r)) for r in rows]  # noqa: E731
    count = [len(r) for r in cls] if count is None else count
    _hand[0] += 1
    name = "hand%d" % _hand[0]
    mcases.BUILDERS[name] = lambda: mcases.register(name, owners, ti, tc, count, pad(cls, 0), pad(score, 0.0), cap)
    return mcases.labels(name), mcases.found(name), mcases.truth(name)


def brute(name, min_points=1, min_truth_points=1):
    """The rule with a Python set per (row, instance)."""
    c = mcases.get(name)
    planes, cap, NC = c["planes"], c["cap"], mcases.NUM_CLASS
    G = max(int(t.max(initial=0)) for t in c["truth_instance"])
    S = len(c["owners"])
    ov, jm = np.full((S, cap), -np.inf), np.full((S, cap), -1)
    npos = np.zeros(65, np.int64)
    for s in range(S):
        o, t, k = c["owners"][s], c["truth_instance"][s], c["truth_class"][s]
        pred = [set(np.nonzero(o == r)[0]) for r in range(cap)]
        inst = [set(np.nonzero(t == g + 1)[0]) for g in range(G)]
        klass = [int(k[min(i)]) if i else -1 for i in inst]
        for g in range(G):
            if len(inst[g]) >= min_truth_points:
                if 0 <= klass[g] < NC:
                    npos[klass[g]] += 1
                elif not 0 <= klass[g] < 64:
                    npos[64] += 1
        for r in range(min(max(int(planes["count"][s]), 0), cap)):
            cl = int(planes["cls"][s, r])
            if len(pred[r]) < min_points or not 0 <= cl < NC:
                continue
            for g in range(G):
                if len(inst[g]) >= min_truth_points and klass[g] == cl:
                    iou = np.float64(len(pred[r] & inst[g])) / np.float64(len(pred[r] | inst[g]))
                    if iou > ov[s, r]:
                        ov[s, r], jm[s, r] = iou, g
    return ov, jm, npos


@pytest.mark.parametrize("name,least", [("lengths", (1, 1)), ("empty", (1, 1)), ("empty", (20, 30)), ("waves", (1, 1))])
def test_against_python_sets(name, least):
    want = mcases.want(name, *least)
    ov, jm, npos = brute(name, *least)
    assert np.array_equal(want["ovmax"].view(np.uint64), ov.view(np.uint64))
    assert np.array_equal(want["jmax"], jm) and np.array_equal(want["npos"], npos)
    assert np.isfinite(ov).any() and (jm < 0).any()
    assert np.array_equal(want["key"] == NONE, ~np.isfinite(ov) & (want["key"] == NONE))
    lab = mcases.labels(name)
    S, cap = lab.points.shape
    assert want["inter"].sum((0, 2)).tolist() == [
        int(sum(((o == r) & (t > 0)).sum() for o, t in zip(mcases.get(name)["owners"], mcases.get(name)["truth_instance"])))
        for r in range(cap)]


def test_per_class_scores_and_a_class_out_of_range():
    want, planes = mcases.want("scores"), mcases.get("scores")["planes"]
    cls = planes["cls"]
    det = want["key"] != NONE
    assert det.any() and (~det).any() and ((cls == mcases.NUM_CLASS) | (cls < 0)).any()
    assert not det[(cls < 0) | (cls >= mcases.NUM_CLASS)].any()
    s, r = np.nonzero(det)
    assert np.array_equal(want["score"][s, r], planes["score"][s, r, cls[s, r]])
    assert not want["score"][~det].any()


def _ap(parts, thresholds=(0.25, 0.5), **least):
    calc = ME.MaskAPCalculator(thresholds)
    matches = [calc.step(*p, **least) for p in parts]
    return calc, matches


# four instances of 10 points each, then 10 unannotated points
TI = [1] * 10 + [2] * 10 + [3] * 10 + [4] * 10 + [0] * 10


def test_perfect_masks_have_ap_one():
    owners = [g - 1 for g in TI]
    calc, (m,) = _ap([hand([owners], [TI], [[0] * 10 + [0] * 10 + [2] * 10 + [5] * 10 + [-1] * 10],
                           [[0, 0, 2, 5]], [[0.9, 0.8, 0.7, 0.6]])])
    assert m.ovmax.tolist() == [[1.0] * 4] and m.jmax.tolist() == [[0, 1, 2, 3]]
    assert m.npos[[0, 2, 5]].tolist() == [2, 1, 1] and m.npos.sum() == 4
    for metrics in calc.compute_metrics():
        assert [metrics["%d Average Precision" % c] for c in (0, 2, 5)] == [1.0, 1.0, 1.0]
        assert metrics["mAP"] == 1.0 and metrics["AR"] == 1.0
    assert calc.mean_iou() == 1.0 and int(calc.no_class) == 0


def test_duplicate_is_one_false_positive_and_missing_class_is_zero():
    # rows 0 / 1 split instance 1 six to four (row 1 scores lower: the duplicate), row 2 is instance 2;
    # instance 3 of class 2 has no detection
    owners = [0] * 6 + [1] * 4 + [2] * 10 + [-1] * 30
    calc, (m,) = _ap([hand([owners], [TI], [[0] * 20 + [2] * 10 + [0] * 10 + [-1] * 10],
                           [[0, 0, 0]], [[0.9, 0.8, 0.7]])])
    assert m.ovmax.tolist() == [[0.6, 0.4, 1.0]] and m.jmax.tolist() == [[0, 0, 1]]
    assert m.npos[[0, 2]].tolist() == [3, 1]
    (rec, prec, ap), (_, _, ap50) = calc.eval_det()
    # class 0 at 0.25: TP, FP (instance 1 is taken), TP of 3 truths
    assert prec[0].tolist() == [1.0, 0.5, 2 / 3] and rec[0].tolist() == [1 / 3, 1 / 3, 2 / 3]
    assert ap[0] == pytest.approx(1 / 3 * 1.0 + 1 / 3 * (2 / 3), abs=1e-15)
    assert ap[2] == 0 and ap50[2] == 0 and rec[2] == 0
    # at 0.5 the duplicate's 0.4 is below the threshold as well: still one false positive
    assert ap50[0] == ap[0]
    assert calc.mean_iou() == pytest.approx((0.6 + 0.4 + 1.0) / 3, abs=1e-15)


def test_detection_on_an_instance_of_no_class_is_a_false_positive():
    owners = [0] * 10 + [1] * 10 + [-1] * 30
    calc, (m,) = _ap([hand([owners], [TI], [[-1] * 10 + [3] * 10 + [40] * 10 + [3] * 10 + [-1] * 10],
                           [[3, 3]], [[0.9, 0.8]])])
    # row 0 covers instance 1 exactly, but that instance has no class: its best is a class-3 instance it misses
    assert m.ovmax.tolist() == [[0.0, 1.0]] and m.jmax.tolist() == [[1, 1]]
    assert m.npos[3] == 2 and m.npos[64] == 1 and m.npos.sum() == 3  # class 40 >= NC: counted nowhere
    assert int(calc.no_class) == 1
    (rec, prec, ap), _ = calc.eval_det()
    assert prec[3].tolist() == [0.0, 0.5] and rec[3].tolist() == [0.0, 0.5] and ap[3] == 0.25
    assert sorted(ap) == [3]


def test_min_points_and_min_truth_points_at_the_size():
    owners = [0] * 7 + [-1] * 3 + [1] * 10 + [-1] * 30
    parts = hand([owners], [TI], [[1] * 50], [[1, 1]], [[0.9, 0.8]])
    for least, det in ((6, True), (7, True), (8, False)):
        m = ME.match_masks(*parts, min_points=least)
        assert (m.key[0, 0] == 1) == det and (m.ovmax[0, 0] == 0.7) == det and m.key[0, 1] == 1
        assert (m.jmax[0, 0] == 0) == det and m.npos[1] == 4
    for least, big in ((9, 4), (10, 4), (11, 0)):
        m = ME.match_masks(*parts, min_truth_points=least)
        assert m.npos[1] == big and np.isfinite(m.ovmax[0, :2]).all() == (big > 0) and (m.key[0, :2] == 1).all()
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="min_points"):
            ME.match_masks(*parts, min_points=bad)
        with pytest.raises(ValueError, match="min_truth_points"):
            ME.match_masks(*parts, min_truth_points=bad)


def test_mixed_class_instance_takes_its_lowest_index_point():
    tc = [4] + [9] * 9 + [9] + [4] * 9 + [-1] * 30
    m = ME.match_masks(*hand([[0] * 10 + [1] * 10 + [-1] * 30], [TI], [tc], [[4, 4]], [[0.5, 0.5]]))
    assert m.klass.tolist() == [[4, 9, -1, -1]] and m.size.tolist() == [[10] * 4]
    assert m.ovmax.tolist() == [[1.0, 0.0]] and m.jmax.tolist() == [[0, 0]]
    assert m.npos[4] == 1 and m.npos[9] == 1 and m.npos[64] == 2


def test_tie_between_two_instances_goes_to_the_lower():
    # row 0 takes five points of instance 2 and five of instance 1: 5 / 15 both ways
    owners = [0] * 5 + [-1] * 5 + [0] * 5 + [-1] * 35
    m = ME.match_masks(*hand([owners], [TI], [[2] * 50], [[2]], [[0.5]]))
    assert m.inter[0, 0].tolist() == [5, 5, 0, 0] and m.ovmax[0, 0] == 5 / 15 and m.jmax[0, 0] == 0


def test_scans_never_interact_and_slots_advance():
    one = ([0] * 10 + [-1] * 40, TI, [0] * 50)
    two = ([-1] * 10 + [0] * 10 + [-1] * 30, TI, [0] * 50)
    both = hand([one[0], two[0]], [one[1], two[1]], [one[2], two[2]], [[0], [0]], [[0.9], [0.8]])
    calc, (m, _) = _ap([both, hand([one[0]], [one[1]], [one[2]], [[0]], [[0.7]])])
    assert m.jmax.tolist() == [[0], [1]] and calc._gt_slots == 2 * 4 + 4 and calc.scan_cnt == 3
    assert np.concatenate(calc._gt_id).tolist() == [0, 4 + 1, 8]
    assert calc._npos[0] == 12 and calc.compute_metrics()[0]["0 Average Precision"] == pytest.approx(3 / 12)


def test_point_truth_refusals():
    lab, found, truth = hand([[0] * 10 + [-1] * 40], [TI], [[0] * 50], [[0]], [[0.9]])
    with pytest.raises(ValueError, match="G = 0"):
        ME.PointTruth(["a"], [[0, 0, -3]], [[1, 1, 1]], None)
    with pytest.raises(ValueError, match="instance ids for"):
        ME.PointTruth(["a"], [[1, 2]], [[1]], None)
    with pytest.raises(ValueError, match="1-D integer"):
        ME.PointTruth(["a"], [[1.0, 2.0]], [[1, 1]], None)
    with pytest.raises(ValueError, match="1 names, 2 instance"):
        ME.PointTruth(["a"], [[1], [1]], [[1]], None)
    with pytest.raises(ValueError, match="table entries"):
        ME.PointTruth(["a", "b"], [[1 << 29], [1]], [[0], [0]], None)
    big = ME.PointTruth(["a"], [[1 << 20]], [[0]], None)
    with pytest.raises(ValueError, match="table entries"):
        big.check(big, cap=4096)
    big.check(big, cap=2045)  # 2^20 * 2048 entries: the most
    short = ME.PointTruth(truth.names, [TI[:-1]], [[0] * 49], None)
    with pytest.raises(ValueError, match="length mismatch"):
        short.check(lab)
    with pytest.raises(ValueError, match="length mismatch"):
        ME.match_masks(lab, found, short)
    other = ME.PointTruth(["elsewhere"], [TI], [[0] * 50], None)
    with pytest.raises(ValueError, match="'elsewhere'"):
        other.check(lab)
    with pytest.raises(ValueError, match="2 scans of truth"):
        ME.PointTruth(["a", "b"], [TI, TI], [[0] * 50] * 2, None).check(lab)
    with pytest.raises(ValueError, match="PointLabels"):
        ME.match_masks(found, found, truth)


def test_from_scannet_maps_nyu40_ids(tmp_path):
    SD = importlib.import_module("3dioumatch_amd.votenet.scannet_data")
    ins = np.array([0, 1, 1, 2, 3, 3], np.uint32)
    sem = np.array([0, 3, 3, 39, 1, 40], np.uint32)  # nyu40 3 -> class 0, 39 -> 17, 1 and 40: no class
    np.save(tmp_path / "room_ins_label.npy", ins)
    np.save(tmp_path / "room_sem_label.npy", sem)
    truth = ME.PointTruth.from_scannet(str(tmp_path), ["room"], None)
    assert truth.G == 3 and truth.instance.tolist() == [0, 1, 1, 2, 3, 3] and truth.instance.dtype == np.int32
    assert truth.klass.tolist() == [-1, 0, 0, 17, -1, -1]
    assert SD.NYU40IDS[0] == 3 and SD.NYU40IDS[17] == 39
    with pytest.raises(ValueError, match="missing"):
        ME.PointTruth.from_scannet(str(tmp_path), ["absent"], None)


def test_exports_and_constants():
    for name in ("MaskAPCalculator", "MaskMatch", "PointTruth", "host_match_masks", "match_masks"):
        assert getattr(V, name) is getattr(ME, name)
    assert issubclass(ME.MaskAPCalculator, V.DeviceAPCalculator)
    L = importlib.import_module("3dioumatch_amd._lib")
    for name in ("scene_mask_scratch_bytes", "scene_mask_overlap", "scene_mask_match"):
        assert name in L._LOADER_SIGNATURES and name not in L.EXPORTS and hasattr(L.lib, name)
    for S, cap, G in ((1, 1, 1), (3, 256, 70), (1, 4096, 1000)):  # a host function
        assert ME.mask_scratch_bytes(S, cap, G) == 4 * ME.table_entries(S, cap, G) == 4 * S * G * (cap + 3)
    assert ME.mask_scratch_bytes(0, 4, 4) == ME.mask_scratch_bytes(4, 0, 4) == ME.mask_scratch_bytes(4, 4, 0) == 0
    header = open(os.path.join(ROOT, "include", "mask_eval_hip.h")).read()
    assert "#define MASK_BLOCK %d " % ME.MASK_BLOCK in header
    assert "#define MASK_MERGE_ROUNDS %d " % ME.MASK_MERGE_ROUNDS in header
    assert "#define MASK_MAX_CLASS %d " % ME.EVAL_MAX_CLASS in header
    assert ME.MASK_BLOCK == cases.B  # one max_blocks serves both launches


def _tool():
    spec = importlib.util.spec_from_file_location("tools_detect_masks", os.path.join(ROOT, "tools", "detect.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tool_flags():
    tool = _tool()
    p = tool.mask_flags(tool.parser())
    assert vars(p.parse_args([]))["truth"] is None and "truth" not in vars(tool.parser().parse_args([]))
    assert tool.mask_scoring(p.parse_args(["x.npy", "--out", "o", "--labels"])) is None
    got = tool.mask_scoring(p.parse_args(["x.npy", "--out", "o", "--labels", "--truth", "d", "--mask-iou", "0.3"]))
    assert got == ("d", (0.3,), 1)
    got = tool.mask_scoring(p.parse_args(["x.npy", "--out", "o", "--labels", "--truth", "d", "--mask-min-points", "50"]))
    assert got == ("d", (0.25, 0.5), 50)
    for argv in (["x.npy", "--truth", "d"], ["x.npy", "--out", "o", "--labels", "--mask-iou", "0.5"],
                 ["x.npy", "--out", "o", "--labels", "--mask-min-points", "3"],
                 ["x.npy", "--out", "o", "--labels", "--truth", "d", "--mask-min-points", "0"]):
        with pytest.raises(SystemExit):
            tool.mask_scoring(p.parse_args(argv))
