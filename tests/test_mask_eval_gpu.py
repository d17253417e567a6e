"""The mask matching on the MI355X against host_match_masks, bit for bit: every shared case in both
overlap forms (scan lengths around the workgroup, an empty scan, G around the match wave's stride, the
wave-merge edges, per-class scores), the least-points arguments, a random cloud through the real
label_points (twice, cull on and off), dirty buffers with a guard tail, the refusals of the two entry
points, no synchronising call in a step, and MaskAPCalculator over two steps against its host path."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import label_points_cases as cases
import mask_eval_cases as mcases
from conftest import load_pkg

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
INVALID = 1  # hipErrorInvalidValue
TAIL = 64    # elements behind every pre-filled buffer: nothing may be written there
INTS = ("inter", "size", "klass", "jmax", "key", "npos")

load_pkg()
ME = importlib.import_module("3dioumatch_amd.votenet.mask_eval")
PL = importlib.import_module("3dioumatch_amd.votenet.point_labels")
SC = importlib.import_module("3dioumatch_amd.votenet.scan_data")


def _assert_same(got, want, what=""):
    for k in INTS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)
    assert got["ovmax"].dtype == np.float64
    assert np.array_equal(got["ovmax"].view(np.uint64), want["ovmax"].view(np.uint64)), (what, "ovmax")
    assert np.array_equal(got["score"].view(np.uint32), want["score"].view(np.uint32)), (what, "score")


def _device(name, merge=ME.MERGE, buffers=None, **least):
    m = ME.match_masks(mcases.labels(name, DEV), mcases.found(name, DEV), mcases.truth(name, DEV), merge=merge,
                       buffers=buffers, **least)
    assert all(torch.is_tensor(getattr(m, k)) and getattr(m, k).device == DEV for k in m.FIELDS)
    return m.host()


@pytest.mark.parametrize("merge", [True, False], ids=["merged", "plain"])
@pytest.mark.parametrize("name", mcases.NAMES)
def test_cases_bit_for_bit(name, merge):
    want = mcases.want(name)
    _assert_same(_device(name, merge), want, name)
    assert np.isfinite(want["ovmax"]).any() and (want["inter"] > 0).any()


def test_the_cases_hold_what_they_are_for():
    B = ME.MASK_BLOCK
    assert [len(o) for o in mcases.get("lengths")["owners"]] == [1, B - 1, B, B + 1, 3 * B + 1]
    assert [len(o) for o in mcases.get("empty")["owners"]] == [300, 0, 77]
    assert not mcases.want("empty")["size"][1].any() and mcases.want("empty")["size"][2].any()
    assert [mcases.truth("g%d" % G).G for G in mcases.G_VALUES] == list(mcases.G_VALUES)
    w = mcases.get("waves")
    o, t = w["owners"][0], w["truth_instance"][0]
    keys = lambda a, b: len(set(zip(o[a:b][(o[a:b] >= 0) & (t[a:b] > 0)], t[a:b][(o[a:b] >= 0) & (t[a:b] > 0)])))  # noqa: E731
    assert keys(0, 64) == 1 and keys(64, 128) == 64 > ME.MASK_MERGE_ROUNDS
    assert keys(3 * B, 3 * B + 64) == 6 > ME.MASK_MERGE_ROUNDS  # six runs: two are left to per-lane atomics
    assert (o[B - 40:B + 90] == 2).all() and (t[B - 40:B + 90] == 2).all()  # over a wave and a workgroup boundary
    last = slice(2 * B + 64, 2 * B + 128)
    assert ((o[last] >= 0) & (t[last] > 0)).tolist() == [False] * 63 + [True]


def test_least_points_on_the_device():
    for least in ((3, 40), (40, 3)):
        _assert_same(_device("lengths", min_points=least[0], min_truth_points=least[1]), mcases.want("lengths", *least))
    a, b, c = mcases.want("lengths"), mcases.want("lengths", 3, 40), mcases.want("lengths", 40, 3)
    assert not np.array_equal(a["key"], c["key"]) and not np.array_equal(a["npos"], b["npos"])


def _filled(shape, dtype, byte):
    n = int(np.prod(shape))
    whole = torch.empty(n + TAIL, dtype=dtype, device=DEV)
    whole.view(torch.uint8).fill_(byte)
    return whole[:n].view(shape), whole, n


@pytest.mark.parametrize("byte", [0x7F, 0xFF], ids=["0x7f", "nan_and_minus_one"])
@pytest.mark.parametrize("name", ["waves", "empty", "g65"])
def test_dirty_buffers(name, byte):
    """every buffer the bindings would allocate arrives filled: 0x7F bytes, or 0xFF bytes (a NaN as
    float64 and float32, -1 as an integer); npos alone is added to and starts at zero"""
    c = mcases.get(name)
    S, cap, G = len(c["owners"]), c["cap"], mcases.truth(name).G
    given, wholes = {}, []
    for k, shape, dtype in (("scratch", (ME.table_entries(S, cap, G),), torch.int32), ("ovmax", (S, cap), torch.float64),
                            ("jmax", (S, cap), torch.int32), ("score", (S, cap), torch.float32),
                            ("key", (S, cap), torch.int16), ("klass", (S, G), torch.int32)):
        given[k], whole, n = _filled(shape, dtype, byte)
        wholes.append((k, whole, n))
    got = _device(name, buffers=given)
    for k, whole, n in wholes:
        assert (whole[n:].view(torch.uint8) == byte).all(), "%s: written behind its end" % k
    _assert_same(got, mcases.want(name), name)
    # npos is documented as accumulated
    npos = torch.arange(65, dtype=torch.int64, device=DEV)
    again = _device(name, buffers={"npos": npos})
    assert np.array_equal(again["npos"], mcases.want(name)["npos"] + np.arange(65))


def _random_through_label_points():
    g = np.random.default_rng(97)
    cloud = cases._room(g, 20000)
    planes = cases._planes(1, 32, 0)
    cases._fill_random(planes, 0, 25, g, 0)
    planes["box"][0, :25, 3:6] *= np.float32(0.5)
    planes["cls"][0, :25] = g.integers(0, 6, 25)
    cell = (np.floor((cloud[:, 0] + 2.0) / 0.8).clip(0, 4) * 8 + np.floor(cloud[:, 1] + 2.0).clip(0, 3) * 2 +
            (cloud[:, 2] >= 1.0)).astype(np.int64)  # 5 x 4 x 2 = 40 instances
    ti = np.where(g.random(len(cloud)) < 0.1, 0, cell + 1)
    tc = cell % 7 - 1
    key = mcases.register("random", [np.full(len(cloud), -1)], [ti], [tc], planes["count"], planes["cls"],
                          planes["score"], 32)
    c = cases.get(key)
    c["planes"]["box"].setflags(write=True)
    c["planes"]["box"][:] = planes["box"]
    c["planes"]["box"].setflags(write=False)
    mcases._keys["random"] = key
    store = SC.ScanStore([cloud], DEV, "scannet", names=c["names"])
    return store, mcases.found("random", DEV), mcases.truth("random", DEV), mcases.truth("random")


def test_random_cloud_through_label_points():
    store, found, truth, host_truth = _random_through_label_points()
    assert host_truth.G == 40 and len(host_truth.instance) == 20000
    runs = []
    for cull in (True, False, True):
        labels = PL.label_points(found, store, cull=cull)
        runs.append((labels, ME.match_masks(labels, found, truth).host()))
    labels, first = runs[0]
    for _, other in runs[1:]:
        _assert_same(other, first, "second run / cull off")
    h = labels.host()
    assert (h["points"] > 0).sum() >= 10 and (h["instance"] >= 0).mean() > 0.1
    want = ME.host_match_masks(h["instance"], h["points"], found.planes(), host_truth, found.num_class)
    _assert_same(first, want, "random")
    assert (np.isfinite(want["ovmax"]) & (want["ovmax"] > 0)).sum() >= 5


def test_step_does_not_synchronise():
    parts = (mcases.labels("noisy0", DEV), mcases.found("noisy0", DEV), mcases.truth("noisy0", DEV))
    calc = ME.MaskAPCalculator()
    calc.step(*parts)  # warm-up
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        calc.step(*parts)
        ME.match_masks(*parts, merge=not ME.MERGE)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    assert calc.scan_cnt == 6 and len(calc.compute_metrics()) == 2


def test_two_steps_equal_the_host_path():
    """the tolerance test_eval_device_gpu.py holds DeviceAPCalculator to against eval_det: atol 1e-12"""
    dev, host = ME.MaskAPCalculator((0.25, 0.5)), ME.MaskAPCalculator((0.25, 0.5))
    for name in ("noisy0", "noisy1"):
        dev.step(mcases.labels(name, DEV), mcases.found(name, DEV), mcases.truth(name, DEV), min_truth_points=5)
        host.step(mcases.labels(name), mcases.found(name), mcases.truth(name), min_truth_points=5)
    assert dev.scan_cnt == host.scan_cnt == 5 and dev._gt_slots == host._gt_slots == 3 * 12 + 2 * 9
    assert np.array_equal(dev._npos.cpu().numpy(), host._npos) and int(dev.no_class) == int(host.no_class) > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        got, want = dev.compute_metrics(), host.compute_metrics()
    partial = False
    for g, w in zip(got, want):
        assert list(g) == list(w)
        print({k: (float(g[k]), float(w[k])) for k in w})
        np.testing.assert_allclose([g[k] for k in w], [w[k] for k in w], rtol=0, atol=1e-12, equal_nan=True)
        partial |= any(0 < v < 1 for k, v in w.items() if k.endswith("Average Precision"))
    assert partial  # ordering, first claim and false positives were exercised
    with np.errstate(invalid="ignore", divide="ignore"):
        curves, host_curves = dev.eval_det(), host.eval_det()
    for (r, p, a), (wr, wp, wa) in zip(curves, host_curves):
        assert sorted(a) == sorted(wa)
        for c in wa:
            np.testing.assert_allclose(np.asarray(r[c]), np.asarray(wr[c]), rtol=0, atol=1e-12, equal_nan=True)
            np.testing.assert_allclose(np.asarray(p[c]), np.asarray(wp[c]), rtol=0, atol=1e-12, equal_nan=True)
    np.testing.assert_allclose(dev.mean_iou(), host.mean_iou(), rtol=0, atol=1e-12)


def test_tool_scores_masks_from_a_prepared_folder(tmp_path, capsys):
    import importlib.util
    import os
    SD = importlib.import_module("3dioumatch_amd.votenet.scannet_data")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("tools_detect_mask_gpu", os.path.join(root, "tools", "detect.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    c = mcases.get("noisy0")
    for name, ti, tc in zip(c["names"], c["truth_instance"], c["truth_class"]):
        np.save(tmp_path / (name + "_ins_label.npy"), ti.astype(np.uint32))
        np.save(tmp_path / (name + "_sem_label.npy"), np.where(tc >= 0, SD.NYU40IDS[np.maximum(tc, 0)], 0).astype(np.uint32))
    labels, found = mcases.labels("noisy0", DEV), mcases.found("noisy0", DEV)
    got = tool.score_masks(found, labels, (str(tmp_path), (0.25, 0.5), 5), DEV)
    assert "mask IoU 0.25" in capsys.readouterr().out
    host = ME.MaskAPCalculator((0.25, 0.5))
    host.step(mcases.labels("noisy0"), mcases.found("noisy0"), mcases.truth("noisy0"), min_points=5, min_truth_points=5)
    with np.errstate(invalid="ignore", divide="ignore"):
        want = host.compute_metrics()
    for g, w in zip(got, want):
        assert list(g) == list(w)
        np.testing.assert_allclose([g[k] for k in w], [w[k] for k in w], rtol=0, atol=1e-12, equal_nan=True)


def test_refusals_without_a_launch():
    _L = importlib.import_module("3dioumatch_amd._lib")
    name = "empty"
    lab, found, truth = mcases.labels(name, DEV), mcases.found(name, DEV), mcases.truth(name, DEV)
    S, cap, G = 3, lab.cap, truth.G
    d = truth.dev
    scratch = torch.zeros(ME.table_entries(S, cap, G) + 2, dtype=torch.int32, device=DEV)
    good = dict(offset=d["offset"], count=d["count"], max_blocks=2, instance=lab.instance, truth_instance=d["instance"],
                truth_class=d["klass"], scratch=scratch, S=S, cap=cap, G=G, merge=True, clear=True)

    def call(entry, record):
        return getattr(_L.lib, entry)(ctypes.byref(record), _L.current_stream_ptr(DEV))

    assert call("scene_mask_overlap", ME.overlap_record(**good)) == 0
    for change in (dict(S=0), dict(S=65536), dict(cap=0), dict(G=0), dict(max_blocks=0), dict(scratch=scratch[1:]),
                   dict(scratch=scratch[:ME.table_entries(S, cap, G) - 1]), dict(cap=1 << 30, G=1 << 10)):
        assert call("scene_mask_overlap", ME.overlap_record(**dict(good, **change))) == INVALID, change
    record = ME.overlap_record(**good)
    record.instance = None
    assert call("scene_mask_overlap", record) == INVALID
    out = ME.match_gpu(lab.rows, torch.zeros((S, cap), dtype=torch.int32, device=DEV),
                       torch.zeros((S, cap), dtype=torch.float32, device=DEV), lab.points, scratch, G, 18)
    args = (lab.rows, out["jmax"], out["score"], lab.points, scratch, G, 18, 1, 1, out)
    assert call("scene_mask_match", ME.match_record(*args)) == 0
    for at, value in ((5, 0), (6, 0), (7, 0), (8, 0)):  # G, NC, min_points, min_truth_points
        bad = list(args)
        bad[at] = value
        assert call("scene_mask_match", ME.match_record(*bad)) == INVALID, at
    record = ME.match_record(*args)
    record.npos = None
    assert call("scene_mask_match", record) == INVALID
    assert _L.lib.scene_mask_overlap(None, None) == INVALID and _L.lib.scene_mask_match(None, None) == INVALID
    torch.cuda.synchronize()
