"""The NMS across the cuts on the MI355X: scene_detections_merge_nms against host_merge_nms bit for
bit -- every hand-made case under every admitted setting, the crowded seeded cases (a hole in the
adjacency, K across a wave, rows with more partners than the kernel records, more candidates than a
workgroup has threads) -- with guard words behind the merged arena and the scratch, twice, and on
scratch and output pre-filled with each fill of dirty_memory; the refusals; and detect_tiled(...,
seam_nms=True) end to end against host_merge_nms of detect() on the tiles, with its invariants."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import dirty_memory
from conftest import load_pkg
from seam_nms_cases import HAND, SETTINGS, hand_case, large_case, random_case, run_host, tables

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GUARD = 64  # words behind the merged arena; GUARD / 2 doubles behind the scratch
# dims, old_type, same_class: same_class in 3-D only
ALL_SETTINGS = [dict(SETTINGS, dims=d, old_type=o, same_class=c)
                for d in (3, 2) for o in (0, 1) for c in ((0, 1) if d == 3 else (0,))]


def _mods():
    load_pkg()
    return (importlib.import_module("3dioumatch_amd.votenet"),
            importlib.import_module("3dioumatch_amd.votenet.scan_data"),
            importlib.import_module("3dioumatch_amd.votenet.scan_tiles"),
            importlib.import_module("3dioumatch_amd.votenet.detect"))


def _arena_of(planes, layout_fn, *dims):
    layout, words = layout_fn(*dims)
    arena = np.zeros(words, np.float32)
    for name, (at, shape) in layout.items():
        flat = np.ascontiguousarray(planes[name]).reshape(-1)
        arena[at:at + flat.size] = flat.view(np.float32) if flat.dtype == np.int32 else flat
    return torch.from_numpy(arena).to(DEV)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Case(object):
    """A tile arena and its tables on the device, run under any settings into guarded buffers."""

    def __init__(self, planes, tab, NC):
        _, _, _, self.D = _mods()
        self.planes, self.tab, self.NC = planes, tab, NC
        self.T, self.K = planes["proposal"].shape
        self.S, self.max_tiles = len(tab["first"]), int(tab["tiles"].max())
        self.cap = self.max_tiles * self.K + 3  # three rows more than the scan's tiles can fill
        self.layout, self.words = self.D.merged_layout(self.S, self.cap, NC)
        self.arena = _arena_of(planes, self.D.arena_layout, self.T, self.K, NC)
        self.dev = {k: _dev(tab[k]) for k in ("first", "tiles", "core", "iy", "ix", "reach")}
        self.doubles = (self.D.seam_scratch_bytes(self.S, self.T, self.K, self.max_tiles) + 7) // 8
        assert self.doubles > 0

    def run(self, settings, fill=7.0):
        """the merged arena's words (host, uint32) after a run into buffers pre-filled with `fill`;
        the guard words behind both buffers must be untouched"""
        merged = torch.full((self.words + GUARD,), fill, dtype=torch.float32, device=DEV)
        scratch = torch.full((self.doubles + GUARD // 2,), fill, dtype=torch.float64, device=DEV)
        d = self.dev
        self.D.merge_nms_gpu(merged[:self.words], self.arena, d["first"], d["tiles"], d["core"], d["iy"], d["ix"],
                             d["reach"], self.S, self.T, self.K, self.NC, self.cap, self.max_tiles,
                             settings["thresh"], settings["old_type"], settings["same_class"], settings["dims"],
                             scratch=scratch[:self.doubles])
        host = merged.cpu().numpy().view(np.uint32)
        assert (host[self.words:] == np.array([fill], np.float32).view(np.uint32)[0]).all(), "behind the merged arena"
        behind = scratch[self.doubles:].cpu().numpy().view(np.uint64)
        assert (behind == np.array([fill], np.float64).view(np.uint64)[0]).all(), "behind the scratch"
        return host[:self.words]

    def check(self, settings):
        """device == host bit for bit, plane by plane; twice; and on every dirty fill"""
        info = {}
        want = run_host(self.planes, self.tab, settings, cap=self.cap, info=info)
        got = self.run(settings)
        for name, (at, shape) in self.layout.items():
            ref = np.ascontiguousarray(want[name]).view(np.uint32).reshape(-1)
            assert np.array_equal(got[at:at + ref.size], ref), (name, settings, want["count"],
                                                                  got[:self.S].view(np.int32))
        assert np.array_equal(self.run(settings), got), "the second run"
        for fill, tag in zip(dirty_memory.FILLS, dirty_memory.FILL_IDS):
            assert np.array_equal(self.run(settings, fill), got), tag
        return want, info


# ------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize("NC", [0, 3])
@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_made_cases_are_host_merge_nms(name, NC):
    planes, own, kept, _ = hand_case(name, NC)
    case = Case(planes, tables(), NC)
    want, _ = case.check(own)
    assert want["count"].tolist() == [len(k) for k in kept]
    for settings in ALL_SETTINGS:
        case.check(settings)
    torch.cuda.synchronize()


@pytest.mark.parametrize("NC", [3, 0])
def test_crowded_seams_are_host_merge_nms(NC):
    """3 x 3 tiles without the centre one and 1 x 5 tiles, K = 70 (test_seam_nms.py holds what the case contains)"""
    planes, tab = random_case(NC)
    case = Case(planes, tab, NC)
    for settings in (SETTINGS, dict(SETTINGS, dims=2, same_class=0), dict(SETTINGS, old_type=1),
                     dict(SETTINGS, same_class=0, thresh=0.0625),
                     dict(SETTINGS, thresh=-1.0)):  # below zero: boxes that are apart are partners too (0 > -1)
        want, info = case.check(settings)
        print("settings", settings, "kept", want["count"].tolist(), info)
        assert max(info["rounds"]) >= 3 and max(info["most_above"]) > 4
    torch.cuda.synchronize()


def test_more_candidates_than_a_workgroup_has_threads():
    planes, tab = large_case(0)
    case = Case(planes, tab, 0)
    assert case.max_tiles * case.K > 1024
    want, info = case.check(SETTINGS)
    print("kept", want["count"].tolist(), info)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ refusals
def test_refusals_without_a_launch():
    _, _, _, D = _mods()
    L = importlib.import_module("3dioumatch_amd._lib")
    R = importlib.import_module("3dioumatch_amd.records")
    planes, settings, _, _ = hand_case("corner", 3)
    case = Case(planes, tables(), 3)
    K, cap = case.K, case.cap
    need = D.seam_scratch_bytes(2, 5, K, 4)
    assert need >= 2 * 4 * K * (8 + 4 * 10) and D.seam_scratch_bytes(0, 5, K, 4) == 0
    scratch = torch.zeros(need // 8 + 1, dtype=torch.float64, device=DEV)
    invalid = 1  # hipErrorInvalidValue

    def args(**over):
        a = R.ScanSeamArgs()
        for f, kind in a._fields_:
            if kind is ctypes.c_void_p:
                setattr(a, f, case.arena.data_ptr())
        a.S, a.K, a.NC, a.cap, a.max_tiles = 2, K, 3, cap, 4
        a.thresh, a.old_type, a.same_class, a.dims = 0.25, 0, 1, 3
        a.scratch, a.scratch_bytes = scratch.data_ptr(), need
        for k, v in over.items():
            setattr(a, k, v)
        return a

    call = L.lib.scene_detections_merge_nms
    for over in ({"S": 0}, {"K": 0}, {"K": D.MAX_K + 1, "cap": 8 * D.MAX_K}, {"NC": -1}, {"dims": 1}, {"dims": 4},
                 {"dims": 2}, {"cap": 4 * K - 1}, {"max_tiles": 0}, {"scratch_bytes": need - 1}, {"scratch_bytes": 0},
                 {"scratch": scratch.data_ptr() + 4}):
        assert call(ctypes.byref(args(**over)), None) == invalid, over
    for f, kind in R.ScanSeamArgs._fields_:
        if kind is ctypes.c_void_p:
            assert call(ctypes.byref(args(**{f: None})), None) == invalid, f
    assert call(None, None) == invalid
    assert [f for f, _ in R.ScanSeamArgs._fields_[:21]] == [f for f, _ in R.ScanMergeArgs._fields_]
    assert ctypes.sizeof(R.ScanSeamArgs) == ctypes.sizeof(R.ScanMergeArgs) + 3 * 8 + 8 + 3 * 4 + 4 + 8 + 8

    # the binding
    d = case.dev
    merged = torch.zeros(case.words, dtype=torch.float32, device=DEV)

    def bind(**over):
        kw = dict(merged=merged, tile_arena=case.arena, first=d["first"], tiles=d["tiles"], core=d["core"], iy=d["iy"],
                  ix=d["ix"], reach=d["reach"], S=2, T=5, K=K, NC=3, cap=cap, max_tiles=4, thresh=0.25, old_type=0,
                  same_class=1, dims=3)
        kw.update(over)
        return D.merge_nms_gpu(**kw)

    for match, over in (("cap", {"cap": 4 * K - 1}), ("dims", {"dims": 5}), ("dims", {"dims": 2}),
                        ("iy", {"iy": d["iy"].long()}), ("ix", {"ix": d["ix"][:4]}),
                        ("reach", {"reach": d["reach"][:, :3]}),
                        ("reach", {"reach": d["reach"].cpu()}), ("core", {"core": d["core"].double()}),
                        ("scratch", {"scratch": scratch[:need // 8 - 1]}), ("scratch", {"scratch": scratch.float()}),
                        ("tile arena", {"tile_arena": case.arena[:-1]}), ("merged arena", {"merged": merged[:-1]}),
                        ("K =", {"K": D.MAX_K + 1})):
        with pytest.raises(ValueError, match=match):
            bind(**over)
    bind()  # and as it stands it runs
    torch.cuda.synchronize()
    assert merged[:2].view(torch.int32).tolist() == [1, 3]


# ------------------------------------------------------------------ detect_tiled(seam_nms=True), end to end
def _randomize_bn(module, seed):  # tests/test_scan_detect_gpu.py's
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for bn in module.modules():
            if isinstance(bn, torch.nn.modules.batchnorm._BatchNorm):
                c = bn.num_features
                sign = torch.where(torch.rand(c, generator=g) < 0.2, -1.0, 1.0)
                bn.weight.copy_(sign * (0.5 + torch.rand(c, generator=g)))
                bn.bias.copy_(torch.randn(c, generator=g) * 0.2)
                bn.running_mean.copy_(torch.randn(c, generator=g) * 0.3)
                bn.running_var.copy_(0.3 + torch.rand(c, generator=g) * 2.0)


def _config_dict(cfg, **over):
    cd = {"dataset_config": cfg, "remove_empty_box": False, "use_3d_nms": True, "nms_iou": 0.25,
          "use_old_type_nms": False, "cls_nms": True, "use_iou_for_nms": False, "per_class_proposal": True,
          "conf_thresh": 0.05}
    cd.update(over)
    return cd


@pytest.fixture(scope="module")
def run_setup():
    """tests/test_scan_tiles_gpu.py's: the small detector, 6 synthetic scans of 25 000 rows, 20 000
    points, a confidence threshold at the median objectness"""
    V, SC, ST, D = _mods()
    I = importlib.import_module("3dioumatch_amd.votenet.inference")
    step = importlib.import_module("3dioumatch_amd.votenet.step")
    cfg = V.scannet_config()
    det = step.build_detector(cfg, seed=0).to(DEV)
    _randomize_bn(det, 11)
    det = det.eval()
    store = SC.ScanStore(SC.synthetic_clouds(6, 25000, seed=3, color=False), DEV, "scannet")
    loader = SC.ScanLoader(store, 20000, seed=2)
    engine = I.InferenceEngine(det)
    ep = engine(loader.batch([0, 1], 0)["point_clouds"])
    thresh = float(torch.softmax(ep["objectness_scores"], -1)[:, :, 1].median())
    return engine, store, cfg, thresh


def _overlap(a, b, same_class):
    """the union overlap of two rows' bounds in float64, 3-D; a, b = (corners (8, 3), cls)"""
    lo_a, hi_a = a[0].min(0).astype(np.float64), a[0].max(0).astype(np.float64)
    lo_b, hi_b = b[0].min(0).astype(np.float64), b[0].max(0).astype(np.float64)
    d = np.minimum(hi_a, hi_b) - np.maximum(lo_a, lo_b)
    d = np.where(d > 0, d, 0.0)
    inter = d[0] * d[1] * d[2]
    va, vb = np.prod(hi_a - lo_a), np.prod(hi_b - lo_b)
    with np.errstate(divide="ignore", invalid="ignore"):
        o = inter / (va + vb - inter)
    return o * (1.0 if not same_class or a[1] == b[1] else 0.0)


@pytest.mark.parametrize("per_class", [True, False])
def test_two_by_two_is_host_merge_nms_of_detect_on_the_tiles(run_setup, per_class, tmp_path):
    V, SC, ST, D = _mods()
    engine, store, cfg, thresh = run_setup
    cd = _config_dict(cfg, per_class_proposal=per_class, conf_thresh=thresh)
    tiles = ST.TileStore.from_store(store, (4.5, 3.5), overlap=1.0)  # the 8 m x 6 m rooms: 2 x 2
    assert tiles.tiles.tolist() == [4] * 6 and len(tiles) == 24 and tiles.overlap == 1.0
    loader = SC.ScanLoader(tiles, 20000, seed=2)
    per_tile = V.detect(engine, loader, cd, batch_size=8, counter=3)
    found = V.detect_tiled(engine, loader, cd, batch_size=8, counter=3, seam_nms=True)
    assert torch.equal(found.tiles.arena.view(torch.int32), per_tile.arena.view(torch.int32))
    settings = {"seam": 0.5, "thresh": 0.25, "old_type": 0, "same_class": 1, "dims": 3}
    assert found.seam == settings
    reach = D.seam_reach(tiles.core, 0.5)
    assert np.array_equal(found.reach.view(np.uint32), reach.view(np.uint32))
    tp = per_tile.planes()
    info = {}
    want = D.host_merge_nms(tp, tiles.first, tiles.tiles, tiles.core, tiles.iy, tiles.ix, reach, 0.25, 0, 1, 3,
                            info=info)
    got = found.planes()
    assert found.cap == 4 * found.K
    for name in D.MERGED_PLANES:
        assert got[name].shape == want[name].shape, name
        assert np.array_equal(np.ascontiguousarray(got[name]).view(np.uint32),
                              np.ascontiguousarray(want[name]).view(np.uint32)), name

    # the switch off: today's arena, bit for bit
    plain = V.detect_tiled(engine, loader, cd, batch_size=8, counter=3)
    off = V.detect_tiled(engine, loader, cd, batch_size=8, counter=3, seam_nms=False)
    assert off.seam is None and off.reach is None
    assert torch.equal(off.arena.view(torch.int32), plain.arena.view(torch.int32))
    base = plain.planes()
    ref = D.host_merge(tp, tiles.first, tiles.tiles, tiles.core)
    for name in D.MERGED_PLANES:
        assert np.array_equal(np.ascontiguousarray(base[name]).view(np.uint32),
                              np.ascontiguousarray(ref[name]).view(np.uint32)), name

    # the invariants
    differ = 0
    for s in range(6):
        c = int(got["count"][s])
        rows = [(int(got["tile"][s, r]), int(got["proposal"][s, r])) for r in range(c)]
        plain_rows = {(int(base["tile"][s, r]), int(base["proposal"][s, r])) for r in range(int(base["count"][s]))}
        owned = [bool(ST.in_box(got["box"][s, r, 0:2], tiles.core[rows[r][0]])) for r in range(c)]
        assert {rows[r] for r in range(c) if owned[r]} <= plain_rows   # kept owned rows: rows of the plain merge
        differ += len(set(rows) ^ plain_rows)
        near = lambda t, u: t != u and abs(int(tiles.iy[t]) - int(tiles.iy[u])) <= 1 and \
            abs(int(tiles.ix[t]) - int(tiles.ix[u])) <= 1  # noqa: E731
        for r in range(c):       # no two kept rows of neighbouring tiles are partners
            for q in range(r):
                if near(rows[r][0], rows[q][0]):
                    o = _overlap((got["corners"][s, r], got["cls"][s, r]), (got["corners"][s, q], got["cls"][s, q]), 1)
                    assert not o > 0.25, (s, r, q, o)
        for r in range(c):       # every kept guest has a partner among the candidates
            if owned[r]:
                continue
            t = rows[r][0]
            partners = 0
            for u in range(int(tiles.first[s]), int(tiles.first[s]) + 4):
                if not near(t, u):
                    continue
                for j in range(int(tp["count"][u])):
                    if ST.in_box(tp["box"][u, j, 0:2], reach[u]):
                        o = _overlap((got["corners"][s, r], got["cls"][s, r]),
                                     (tp["corners"][u, j], tp["cls"][u, j]), 1)
                        partners += bool(o > 0.25)
            assert partners > 0, (s, r)
    print("per_class %s: %d rows differ from the plain merge (kept %d, plain %d); %s"
          % (per_class, differ, int(got["count"].sum()), int(base["count"].sum()), info))

    found.save(str(tmp_path))
    with np.load(str(tmp_path / "scan0003.npz")) as f:
        assert int(f["count"]) == got["count"][3] and f["reach"].shape == (4, 4) and float(f["seam"]) == 0.5
        assert float(f["seam_thresh"]) == 0.25 and int(f["seam_dims"]) == 3 and int(f["seam_same_class"]) == 1
        assert int(f["seam_old_type"]) == 0 and f["box"].shape == (int(f["count"]), 7)
    with pytest.raises(ValueError, match="seam"):
        V.detect_tiled(engine, loader, cd, batch_size=8, counter=3, seam_nms=True, seam=-0.5)
    with pytest.raises(ValueError, match="seam"):
        V.detect_tiled(engine, loader, cd, batch_size=8, counter=3, seam=0.5)


def test_seam_nms_is_reproducible_and_does_not_synchronise(run_setup):
    V, SC, ST, D = _mods()
    engine, store, cfg, thresh = run_setup
    cd = _config_dict(cfg, per_class_proposal=False, conf_thresh=thresh)
    tiles = ST.TileStore.from_store(store, (4.5, 3.5), overlap=1.0)
    loader = SC.ScanLoader(tiles, 20000, seed=2)
    first = V.detect_tiled(engine, loader, cd, batch_size=8, counter=1, seam_nms=True)  # warm-up: graphs captured
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            first.arena.cpu()
        except RuntimeError:
            pass
        else:
            pytest.skip("torch.cuda.set_sync_debug_mode('error') does not flag a .cpu() on this build")
        second = V.detect_tiled(engine, loader, cd, batch_size=8, counter=1, seam_nms=True)  # raises nothing
        with pytest.raises(RuntimeError):
            second[0]   # reading is the first synchronising call
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    assert torch.equal(first.arena.view(torch.int32), second.arena.view(torch.int32))
    assert torch.equal(first.tiles.arena.view(torch.int32), second.tiles.arena.view(torch.int32))
    assert second[0]["count"] == first[0]["count"]
