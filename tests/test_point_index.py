"""CPU tests of the point index (votenet/point_index.py): host_point_index against a literal per-row
np.nonzero loop on every shared case, the properties of the rule, PointLabels.index() on the host path
against the old points_of, save(index=True), the tool's flag and the ValueErrors."""
import importlib
import importlib.util
import os

import numpy as np
import pytest

import label_points_cases as label_cases
import point_index_cases as cases
from conftest import ROOT, load_pkg

load_pkg()
V = importlib.import_module("3dioumatch_amd.votenet")
SC = importlib.import_module("3dioumatch_amd.votenet.scan_data")
PL = importlib.import_module("3dioumatch_amd.votenet.point_labels")
PI = importlib.import_module("3dioumatch_amd.votenet.point_index")


def test_constants_follow_the_header():
    text = open(os.path.join(ROOT, "include", "point_index_hip.h")).read()
    for name in ("INDEX_DIGIT_BITS", "INDEX_SEGMENT", "INDEX_TILE"):
        assert "#define %s %d " % (name, getattr(PI, name)) in text, name
    assert PI.INDEX_SEGMENT % PI.INDEX_TILE == 0 and PI.INDEX_TILE % 64 == 0
    assert [PI.passes_of(c) for c in (1, 8191, 8192, 4096 * 1024, PI.INDEX_MAX_CAP)] == [1, 1, 2, 2, 2]
    assert PI.INDEX_MAX_CAP == (1 << 26) - 1
    with pytest.raises(ValueError, match="two digits"):
        PI.passes_of(PI.INDEX_MAX_CAP + 1)
    assert V.PointIndex is PI.PointIndex and V.host_point_index is PI.host_point_index


@pytest.mark.parametrize("case", sorted(cases.CASES))
def test_host_index_equals_the_literal_lists(case):
    c, got = cases.get(case), cases.want(case)
    assert got["start"].dtype == np.int32 and got["order"].dtype == np.int32
    assert got["start"].shape == (len(c["count"]), c["cap"] + 1) and got["order"].shape == c["keys"].shape
    for s, (o, n) in enumerate(zip(c["offset"], c["count"])):
        k = c["keys"][o:o + n]
        order, start = got["order"][o:o + n], got["start"][s]
        at = 0
        for r in range(c["cap"]):
            mine = np.nonzero(k == r)[0]
            assert start[r] == at, (s, r)
            assert np.array_equal(order[at:at + len(mine)], mine), (s, r)
            at += len(mine)
        assert start[c["cap"]] == at
        tail = np.nonzero((k < 0) | (k >= c["cap"]))[0]
        assert np.array_equal(order[at:], tail)


@pytest.mark.parametrize("case", sorted(cases.CASES))
def test_properties_of_the_rule(case):
    c, got = cases.get(case), cases.want(case)
    cap = c["cap"]
    for s, (o, n) in enumerate(zip(c["offset"], c["count"])):
        order, start = got["order"][o:o + n].astype(np.int64), got["start"][s].astype(np.int64)
        assert np.array_equal(np.sort(order), np.arange(n))              # a permutation
        assert start[0] == 0 and (np.diff(start) >= 0).all()            # monotone
        b = cases.buckets(case, s)[order]
        assert (np.diff(b) >= 0).all()                                    # grouped by bucket, the tail last
        same = np.diff(b) == 0
        assert (np.diff(order)[same] > 0).all()                           # every list, and the tail, ascending
        tail = int((b == cap).sum())
        assert start[cap] + tail == n
        assert np.array_equal(np.diff(start), np.bincount(b, minlength=cap + 1)[:cap])


LABEL_CASES = ("sizes", "chunks", "ownership")


def _host_labels(case, prefer="score"):
    c = label_cases.get(case)
    store = SC.ScanStore(c["clouds"], None, "scannet", names=c["names"])
    return store, PL.label_points(label_cases.found(case, label_cases.arena(case)), store, prefer=prefer)


@pytest.mark.parametrize("case", LABEL_CASES)
def test_labels_index_on_the_host_path(case):
    c = label_cases.get(case)
    for prefer in label_cases.PREFERS:
        store, labels = _host_labels(case, prefer)
        old = [[labels.points_of(i, r) for r in range(c["cap"])] for i in range(len(store))]
        unowned = [labels.points_of(i, -1) for i in range(len(store))]
        index = labels.index()
        assert isinstance(index, PI.PointIndex) and labels.index() is index      # built once and kept
        assert isinstance(index.start, np.ndarray) and isinstance(index.order, np.ndarray)
        assert index.start.shape == (len(store), c["cap"] + 1) and index.order.shape == labels.instance.shape
        assert np.array_equal(np.diff(index.start, axis=1), labels.points)
        for i in range(len(store)):
            one = index[i]
            assert np.array_equal(one["start"], index.start[i]) and len(one["order"]) == store.count[i]
            assert index.by_name(c["names"][i])["order"] is not None
            for r in range(c["cap"]):
                assert np.array_equal(index.points_of(i, r), old[i][r]), (i, r)
                now = labels.points_of(i, r)                                      # from the index now
                assert now.dtype == old[i][r].dtype and np.array_equal(now, old[i][r]), (i, r)
            assert np.array_equal(labels.points_of(i, -1), unowned[i])
            assert len(labels.points_of(i, c["cap"])) == 0
            rows, lists = index.lists(i)
            assert np.array_equal(rows, np.nonzero(labels.points[i])[0]) and len(lists) == len(rows)
            for r, l in zip(rows, lists):
                assert np.array_equal(l, old[i][r])
            owned = index.owned(i)
            assert len(owned) == labels.points[i].sum() == index.start[i, c["cap"]]
            assert np.array_equal(np.sort(owned), np.nonzero(labels[i]["instance"] >= 0)[0])
        flat = np.concatenate(store.clouds)
        g = index.gather(flat)
        assert g.shape == flat.shape
        for i, (o, n) in enumerate(zip(store.offset, store.count)):
            assert np.array_equal(g[o:o + n], store.clouds[i][index[i]["order"]])
        with pytest.raises(IndexError):
            index.points_of(0, c["cap"])
        with pytest.raises(IndexError):
            index.points_of(0, -1)
        with pytest.raises(IndexError):
            index[len(store)]
        with pytest.raises(ValueError, match="rows"):
            index.gather(flat[:-1])


def test_save_with_and_without_the_index(tmp_path):
    c = label_cases.get("sizes")
    _, labels = _host_labels("sizes")
    labels.save(str(tmp_path / "plain"))
    plain = {n: open(str(tmp_path / "plain" / (n + "_labels.npz")), "rb").read() for n in c["names"]}
    labels.save(str(tmp_path / "lists"), index=True)
    labels.save(str(tmp_path / "again"))  # with the index built: still the same bytes
    index = labels.index()
    for i, name in enumerate(c["names"]):
        assert open(str(tmp_path / "again" / (name + "_labels.npz")), "rb").read() == plain[name]
        z = np.load(str(tmp_path / "plain" / (name + "_labels.npz")))
        assert sorted(z.files) == ["instance", "min_score", "points", "prefer", "semantic"]
        z = np.load(str(tmp_path / "lists" / (name + "_labels.npz")))
        assert sorted(z.files) == ["instance", "min_score", "order", "points", "prefer", "semantic", "start"]
        rows = int(c["planes"]["count"][i])
        assert z["start"].dtype == np.int32 and z["order"].dtype == np.int32
        assert np.array_equal(z["start"], index.start[i, :rows + 1]) and len(z["start"]) == rows + 1
        assert np.array_equal(z["order"], index[i]["order"])
        assert np.array_equal(np.diff(z["start"]), z["points"])
        for r in range(rows):
            assert np.array_equal(z["order"][z["start"][r]:z["start"][r + 1]], np.nonzero(z["instance"] == r)[0])


def _tool():
    spec = importlib.util.spec_from_file_location("detect_tool", os.path.join(ROOT, "tools", "detect.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_detect_tool_writes_the_lists(tmp_path):
    tool = _tool()
    p = tool.index_flags(tool.mask_flags(tool.parser()))
    assert "labels_index" not in vars(tool.parser().parse_args([])) and vars(p.parse_args([]))["labels_index"] is False
    assert tool.indexing(p.parse_args(["x.npy", "--out", "o", "--labels"])) is False
    assert tool.indexing(tool.parser().parse_args(["x.npy"])) is False
    with pytest.raises(SystemExit, match="goes with --labels"):
        tool.indexing(p.parse_args(["x.npy", "--out", "o", "--labels-index"]))
    c = label_cases.get("ownership")
    raw = SC.ScanStore(c["clouds"], None, "scannet", names=c["names"])
    found = label_cases.found("ownership", label_cases.arena("ownership"))
    flags = p.parse_args(["x.npy", "--out", str(tmp_path), "--labels", "--labels-index"])
    assert tool.indexing(flags) is True
    result = tool.write_labels(found, raw, tool.labeling(flags), flags.out, index=tool.indexing(flags))
    z = np.load(str(tmp_path / "ownership_0_labels.npz"))
    want = PI.host_point_index(result.instance, raw.offset, raw.count, c["cap"])
    assert np.array_equal(z["order"], want["order"])
    assert np.array_equal(z["start"], want["start"][0, :label_cases.OWN_ROWS + 1])


def test_value_errors():
    keys, offset, count = np.array([0, 1, -1, 0], np.int32), np.array([0, 2]), np.array([2, 2])
    PI.host_point_index(keys, offset, count, 2)
    for cap in (0, -1, 1 << 31, 2.0, True, None):
        with pytest.raises(ValueError, match="cap"):
            PI.host_point_index(keys, offset, count, cap)
    with pytest.raises(ValueError, match="flat integer"):
        PI.host_point_index(keys.astype(np.float32), offset, count, 2)
    with pytest.raises(ValueError, match="flat integer"):
        PI.host_point_index(keys.reshape(2, 2), offset, count, 2)
    with pytest.raises(ValueError, match=r"\(S,\)"):
        PI.host_point_index(keys, offset, count[:1], 2)
    with pytest.raises(ValueError, match=r"\(S,\)"):
        PI.host_point_index(keys, offset[:0], count[:0], 2)
    with pytest.raises(ValueError, match="leave"):
        PI.host_point_index(keys, offset, np.array([2, 3]), 2)
    with pytest.raises(ValueError, match="leave"):
        PI.host_point_index(keys, offset, np.array([-1, 2]), 2)
    with pytest.raises(ValueError, match="cap"):
        PI.PointIndex(["a"], count[:1], offset[:1], 0, np.zeros((1, 1), np.int32), np.zeros(2, np.int32))
    # rows of no scan stay -1, and an unsigned plane is read as it is
    got = PI.host_point_index(np.array([3, 0, 9, 0], np.uint32), np.array([1]), np.array([2]), 4)
    assert got["order"].tolist() == [-1, 0, 1, -1] and got["start"].tolist() == [[0, 1, 1, 1, 1]]
