"""The point index on the MI355X: scene_points_index bit-equal to host_point_index on the smallest
shapes at which each mechanism can fail -- scan lengths over the wave, tile and segment edges, key
patterns (a long run, 64 distinct keys per wave, two keys alternating, nothing owned, out-of-range
keys), several scans with an empty one between, the digit edges (cap = 1, the last one-pass cap, two
passes) -- two runs bit-equal, dirty outputs and scratch with a guard tail, poisoned allocations, no
host read inside PointLabels.index() and one at the first index[i], the refusals, and label_points /
detect_tiled end to end."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import dirty_memory
import label_points_cases as label_cases
import point_index_cases as cases
from conftest import load_pkg
from test_label_points_gpu import _config_dict, host_reads, run_setup  # noqa: F401  (run_setup: a fixture)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
INVALID = 1  # hipErrorInvalidValue
TAIL = 64    # words behind every pre-filled buffer: nothing may be written there


def _mods():
    load_pkg()
    return (importlib.import_module("3dioumatch_amd.votenet"),
            importlib.import_module("3dioumatch_amd.votenet.scan_data"),
            importlib.import_module("3dioumatch_amd.votenet.point_labels"),
            importlib.import_module("3dioumatch_amd.votenet.point_index"))


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the shared cases are read-only


def _filled(shape, dtype, byte):
    """(view, whole, n): a tensor of `shape` with TAIL elements behind it, every byte `byte`"""
    n = int(np.prod(shape))
    whole = torch.empty(n + TAIL, dtype=dtype, device=DEV)
    whole.view(torch.uint8).fill_(byte)
    return whole[:n].view(shape), whole, n


def _launch(PI, case, byte=None, exact=True):
    """scene_points_index on the case -> (start, order) as numpy arrays; with `byte` both outputs and
    the scratch arrive filled with it and their guard tails are checked; `exact`: max_segments from the
    counts, else point_index_gpu's own bound"""
    c = cases.get(case)
    S, cap, P = len(c["count"]), c["cap"], len(c["keys"])
    segments = PI.max_segments_of(c["count"]) if exact else None
    given, wholes = {}, []
    if byte is not None:
        need = PI.index_scratch_bytes(S, cap, segments or max(1, -(-P // PI.INDEX_SEGMENT)), P)
        assert need > 0 and need % 8 == 0
        for name, shape, dtype in (("start", (S, cap + 1), torch.int32), ("order", (P,), torch.int32),
                                   ("scratch", (need // 8,), torch.int64)):
            given[name], whole, n = _filled(shape, dtype, byte)
            wholes.append((name, whole, n))
    start, order, _ = PI.point_index_gpu(_dev(c["keys"]), _dev(c["offset"]), _dev(c["count"]), cap,
                                         max_segments=segments, **given)
    torch.cuda.synchronize()
    for name, whole, n in wholes:
        assert (whole[n:].view(torch.uint8) == byte).all(), "%s: written behind its end" % name
    assert start.dtype == torch.int32 and order.dtype == torch.int32
    return start.cpu().numpy(), order.cpu().numpy()


def _assert_equal(case, got):
    want = cases.want(case)
    assert got[0].shape == want["start"].shape and got[1].shape == want["order"].shape
    assert np.array_equal(got[0], want["start"]), case
    assert np.array_equal(got[1], want["order"]), case  # the cases' scans tile the plane: every row is written


# ------------------------------------------------------------------ the launch against numpy
@pytest.mark.parametrize("case", cases.LENGTH_CASES)
def test_scan_lengths(case):
    PI = _mods()[3]
    _assert_equal(case, _launch(PI, case))


@pytest.mark.parametrize("case", cases.PATTERN_CASES)
def test_key_patterns(case):
    PI = _mods()[3]
    _assert_equal(case, _launch(PI, case))


@pytest.mark.parametrize("case", cases.SCAN_CASES)
def test_several_scans(case):
    PI = _mods()[3]
    _assert_equal(case, _launch(PI, case))
    _assert_equal(case, _launch(PI, case, exact=False))  # more segments in the grid than any scan has


@pytest.mark.parametrize("case", cases.DIGIT_CASES)
def test_digit_edges(case):
    PI = _mods()[3]
    assert PI.passes_of(cases.get(case)["cap"]) == (2 if case in ("cap8192", "cap8197") else 1)
    _assert_equal(case, _launch(PI, case))


def test_scratch_is_bounded_by_the_digit_not_by_cap():
    PI = _mods()[3]
    D, P, M = 1 << PI.INDEX_DIGIT_BITS, 1000000, 245
    assert PI.index_scratch_bytes(1, 4096, M, P) == (4 * (M + 1) * 4097 + 7) // 8 * 8  # one pass: the table and the bases
    two = PI.index_scratch_bytes(1, 36 * 1024, M, P)
    assert two == 4 * (M + 1) * D + 12 * P                                   # a 6 x 6 cut: no segments x cap table
    assert PI.index_scratch_bytes(1, PI.INDEX_MAX_CAP, M, P) == two
    for bad in ((0, 8, 1, 10), (1, 0, 1, 10), (1, 8, 0, 10), (1, 8, 1, -1), (1, PI.INDEX_MAX_CAP + 1, 1, 10)):
        assert PI.index_scratch_bytes(*bad) == 0


# ------------------------------------------------------------------ robustness
@pytest.mark.parametrize("case", ["random30", "three", "cap8192", "cap8197"])
def test_two_runs_are_bit_equal_and_dirty_buffers_do_not_matter(case):
    PI = _mods()[3]
    first = _launch(PI, case)
    _assert_equal(case, first)
    for other in [_launch(PI, case)] + [_launch(PI, case, byte=byte) for byte in (0xFF, 0x7F)]:
        assert np.array_equal(first[0], other[0]) and np.array_equal(first[1], other[1])


def test_allocating_wrappers_on_poisoned_allocations():
    PI = _mods()[3]
    for case in ("random30", "cap8197"):
        c = cases.get(case)
        key, offset, count = _dev(c["keys"]), _dev(c["offset"]), _dev(c["count"])
        with dirty_memory.poisoned(dirty_memory.NAN, byte_sites=("index_scratch_bytes",)) as p:
            start, order, scratch = PI.point_index_gpu(key, offset, count, c["cap"])
            torch.cuda.synchronize()
        assert p.byte_count == 1 and scratch.dtype == torch.uint8  # the scratch arrived as 0xFF bytes
        _assert_equal(case, (start.cpu().numpy(), order.cpu().numpy()))


def _labels(case, prefer="score"):
    _, SC, PL, PI = _mods()
    c = label_cases.get(case)
    store = SC.ScanStore(label_cases.clouds(case, 6), DEV, "scannet", names=c["names"])
    found = label_cases.found(case, _dev(label_cases.arena(case)))
    return store, PL.label_points(found, store, prefer=prefer)


@pytest.mark.parametrize("case", ["sizes", "chunks"])
def test_index_without_a_host_read_then_one(case, tmp_path):
    _, SC, PL, PI = _mods()
    c = label_cases.get(case)
    store, labels = _labels(case)
    torch.cuda.synchronize()
    with host_reads() as seen:
        index = labels.index()
        again = labels.index()
    assert seen == [], seen
    assert again is index
    P = int(store.count.sum())
    assert index.start.is_cuda and index.start.dtype == torch.int32 and tuple(index.start.shape) == (len(store), c["cap"] + 1)
    assert index.order.is_cuda and index.order.dtype == torch.int32 and tuple(index.order.shape) == (P,)
    with host_reads() as seen:
        one = index[len(store) - 1]
    assert seen == ["cpu"], seen  # the one copy
    with host_reads() as seen:
        index[0], index.by_name(c["names"][1]), index.points_of(1, 0), index.lists(0), index.owned(1)
    assert seen == [], seen
    instance = labels.instance.cpu().numpy()
    want = PI.host_point_index(instance, store.offset, store.count, c["cap"])
    assert np.array_equal(index.start.cpu().numpy(), want["start"]) and np.array_equal(index.order.cpu().numpy(), want["order"])
    n = int(store.count[-1])
    assert np.array_equal(one["order"], want["order"][-n:]) and np.array_equal(one["start"], want["start"][-1])
    assert np.array_equal(np.diff(want["start"], axis=1), labels.points.cpu().numpy())
    for i in range(len(store)):
        o, k = int(store.offset[i]), int(store.count[i])
        for r in range(c["cap"]):
            old = np.nonzero(instance[o:o + k] == r)[0]
            assert np.array_equal(index.points_of(i, r), old)
            now = labels.points_of(i, r)
            assert now.dtype == old.dtype and np.array_equal(now, old)
    labels.save(str(tmp_path), index=True)
    for i, name in enumerate(c["names"]):
        z = np.load(str(tmp_path / (name + "_labels.npz")))
        rows = int(c["planes"]["count"][i])
        assert np.array_equal(z["start"], want["start"][i, :rows + 1]) and np.array_equal(z["order"], index[i]["order"])


# ------------------------------------------------------------------ refusals
def test_entry_point_refuses_without_a_launch():
    PI = _mods()[3]
    L = importlib.import_module("3dioumatch_amd._lib")
    c = cases.get("three")
    S, cap, P = len(c["count"]), c["cap"], len(c["keys"])
    key, offset, count = _dev(c["keys"]), _dev(c["offset"]), _dev(c["count"])
    segments = PI.max_segments_of(c["count"])
    start, order, scratch = PI.point_index_gpu(key, offset, count, cap, max_segments=segments)
    torch.cuda.synchronize()
    outs = (start, order, scratch)
    before = [t.clone() for t in outs]
    need = PI.index_scratch_bytes(S, cap, segments, P)
    assert need == scratch.numel() and need % 8 == 0

    def refused(**fields):
        a = PI.index_record(key, offset, count, cap, segments, start, order, scratch)
        for k, v in fields.items():
            setattr(a, k, v)
        return L.lib.scene_points_index(ctypes.byref(a), None)

    assert refused() == 0
    bad = [dict(S=0), dict(S=-1), dict(S=65536), dict(cap=0), dict(cap=-3), dict(cap=PI.INDEX_MAX_CAP + 1), dict(max_segments=0), dict(P=-1),
           dict(scratch_bytes=need - 1), dict(scratch_bytes=0), dict(scratch=scratch.data_ptr() + 4), dict(scratch=None),
           dict(cap=1 << 13)]  # two passes need the pair buffers: the same scratch is now too short
    bad += [{name: None} for name in ("key", "offset", "count", "start", "order")]
    torch.cuda.synchronize()
    for fields in bad:
        assert refused(**fields) == INVALID, fields
    assert L.lib.scene_points_index(None, None) == INVALID
    torch.cuda.synchronize()
    for was, now in zip(before, outs):
        assert torch.equal(was, now)  # nothing ran (the accepted call rewrote the same values)
    with pytest.raises(ValueError, match="cap"):
        PI.point_index_gpu(key, offset, count, 0)
    with pytest.raises(ValueError, match="int32"):
        PI.point_index_gpu(key.long(), offset, count, cap)
    with pytest.raises(ValueError, match="offset"):
        PI.point_index_gpu(key, offset.int(), count, cap)


# ------------------------------------------------------------------ end to end
def _assert_index_of_labels(PI, labels, store):
    index = labels.index()
    instance, points = labels.instance.cpu().numpy(), labels.points.cpu().numpy()
    want = PI.host_point_index(instance, store.offset, store.count, labels.cap)
    start, order = index.start.cpu().numpy(), index.order.cpu().numpy()
    assert np.array_equal(start, want["start"]) and np.array_equal(order, want["order"])
    assert np.array_equal(np.diff(start, axis=1), points)
    cloud = store.dev["cloud"]
    g = index.gather(cloud)
    assert g.is_cuda and g.shape == cloud.shape
    g, flat = g.cpu().numpy(), cloud.cpu().numpy()
    for s, (o, n) in enumerate(zip(store.offset, store.count)):
        rows = o + order[o:o + n].astype(np.int64)
        assert np.array_equal(g[o:o + n].view(np.uint32), flat[rows].view(np.uint32))
        owner = np.where(instance[rows] >= 0, instance[rows], labels.cap)
        assert (np.diff(owner) >= 0).all()  # every row's points in ONE run, the unowned last
        assert start[s, labels.cap] == (instance[o:o + n] >= 0).sum()
    return index


@pytest.mark.parametrize("case", ["chunks", "ownership"])
def test_label_points_then_index(case):
    PI = _mods()[3]
    for prefer in label_cases.PREFERS:
        store, labels = _labels(case, prefer)
        index = _assert_index_of_labels(PI, labels, store)
        assert int(index.start.cpu()[:, -1].sum()) > 0


def test_detect_tiled_then_index(run_setup):  # noqa: F811
    V, SC, PL, PI = _mods()
    ST = importlib.import_module("3dioumatch_amd.votenet.scan_tiles")
    engine, raw, cfg, thresh = run_setup
    tiles = ST.TileStore.from_store(raw, (4.5, 3.5), overlap=1.0)  # the 8 m x 6 m rooms: 2 x 2
    tiled = V.detect_tiled(engine, SC.ScanLoader(tiles, 20000, seed=2), _config_dict(cfg, conf_thresh=thresh),
                           batch_size=8, counter=3, seam_nms=True)
    labels = PL.label_points(tiled, tiled.store.source)
    assert labels.cap == 4 * tiled.K
    index = _assert_index_of_labels(PI, labels, raw)
    rows, lists = index.lists(0)
    assert len(rows) > 0 and all(len(l) > 0 for l in lists)
    print("scan 0: %d rows own points, %d points owned of %d" % (len(rows), len(index.owned(0)), raw.count[0]))
