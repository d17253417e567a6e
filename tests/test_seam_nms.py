"""CPU tests of the NMS across the cuts of detect_tiled (votenet/detect.py: host_merge_nms,
seam_reach, seam_settings): the hand-made arenas of seam_nms_cases.py with their kept rows written
out next to the count of the plain merge, the cases where the rule must equal host_merge, the reach
table, the conditions that make the seeded cases of the GPU tests worth comparing, TileStore's new
fields and the flags of tools/detect.py."""
import importlib
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT, load_pkg
from scan_tile_cases import hand_made_tiles
from seam_nms_cases import (CORE, HAND, INF, SETTINGS, hand_case, kept_rows, large_case, random_case, run_host,
                            tables)

load_pkg()
SC = importlib.import_module("3dioumatch_amd.votenet.scan_data")
ST = importlib.import_module("3dioumatch_amd.votenet.scan_tiles")
D = importlib.import_module("3dioumatch_amd.votenet.detect")
V = importlib.import_module("3dioumatch_amd.votenet")


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def same_planes(got, want):
    for name in D.MERGED_PLANES:
        assert got[name].shape == want[name].shape and got[name].dtype == want[name].dtype, name
        assert np.array_equal(bits(got[name]), bits(want[name])), name


# (i) .. (ix) and the variants, by name: the kept rows of scan 0 and the count of the plain merge
EXPECTED = {
    "duplicate": ([(0, 0)], 2),
    "lost": ([(1, 0)], 0),
    "unmatched_guest": ([(1, 0)], 1),
    "chain": ([(0, 0), (3, 0)], 3),
    "corner": ([(1, 0)], 4),
    "classes_apart": ([(0, 0), (1, 0)], 2),
    "classes_together": ([(0, 0)], 2),
    "ties": ([(0, 0), (0, 1), (3, 1)], 6),
    "bounds": ([(1, 0), (1, 1), (2, 0)], 3),
    "stacked_3d": ([(0, 0), (1, 0)], 2),
    "stacked_2d": ([(0, 0)], 2),
    "duplicate_2d": ([(0, 0)], 2),
    "apart_union": ([(0, 0), (1, 0)], 2),
    "apart_old_type": ([(0, 0)], 2),
}


@pytest.mark.parametrize("NC", [0, 3])
@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_made_cases(name, NC):
    planes, settings, kept, plain = hand_case(name, NC)
    assert (kept[0], plain[0]) == EXPECTED[name]  # the literal lists above are the cases' own
    tab = tables()
    info = {}
    got = run_host(planes, tab, settings, info=info)
    base = D.host_merge(planes, tab["first"], tab["tiles"], tab["core"])
    assert base["count"].tolist() == plain
    assert [kept_rows(got, planes, s) for s in (0, 1)] == kept
    assert got["count"].tolist() == [len(k) for k in kept]
    # (ix) the scan of one all-infinite tile is the plain merge's, row for row
    for p in D.MERGED_PLANES:
        assert np.array_equal(bits(got[p][1]), bits(base[p][1])), p
    for p in ("tile", "proposal", "cls", "score", "box", "corners"):  # rows past count are zero
        for s in (0, 1):
            assert not bits(got[p][s, int(got["count"][s]):]).any(), (p, s)
    assert got["tile"].shape == (2, 4 * 6) and got["score"].shape == ((2, 24, NC) if NC else (2, 24))
    want_info = {"lost": (1, 1, 1, 0), "chain": (2, 2, 0, 1), "corner": (6, 1, 0, 3), "unmatched_guest": (0, 0, 0, 0),
                 "bounds": (2, 1, 2, 2)}
    if name in want_info:
        assert tuple(info[k][0] for k in ("pairs", "rounds", "kept_guests", "dropped_owned")) == want_info[name]


def test_cap_and_a_larger_arena():
    planes, settings, kept, _ = hand_case("corner", 3)
    got = run_host(planes, tables(), settings, cap=27)
    assert got["tile"].shape == (2, 27) and got["corners"].shape == (2, 27, 8, 3)
    assert [kept_rows(got, planes, s) for s in (0, 1)] == kept


@pytest.mark.parametrize("NC", [0, 3])
def test_no_partner_pairs_is_the_plain_merge(NC):
    """seam = 0 makes the candidates the owned rows; a threshold no overlap exceeds leaves no pairs"""
    planes, first, tiles, core, _ = hand_made_tiles(NC)
    planes["cls"] %= 3  # that arena's classes run to 17: a key needs the class among the score's columns
    iy, ix = np.array([0, 0, 1, 1, 0], np.int32), np.array([0, 1, 0, 1, 0], np.int32)
    tab = tables(core, iy, ix, first, tiles, seam=0.0)
    assert np.array_equal(bits(tab["reach"]), bits(core))
    info = {}
    got = run_host(planes, tab, dict(SETTINGS, thresh=1.0), info=info)
    assert info["pairs"] == [0, 0]
    same_planes(got, D.host_merge(planes, first, tiles, core))
    # and with pairs (the random boxes of that arena overlap) it is not: the comparison above is not idle
    got = run_host(planes, tab, dict(SETTINGS, thresh=0.0, same_class=0), info=info)
    assert info["pairs"][0] > 0 and got["count"][0] < 7 and got["count"][1] == 5


def test_a_scan_of_one_tile_is_the_plain_merge():
    planes, first, tiles, core, _ = hand_made_tiles(3)
    planes["cls"] %= 3
    one = {k: v[4:] for k, v in planes.items()}
    tab = tables(core[4:], np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32),
                 np.ones(1, np.int32), seam=0.5)
    got = run_host(one, tab, dict(SETTINGS, thresh=0.0, same_class=0))
    same_planes(got, D.host_merge(one, tab["first"], tab["tiles"], tab["core"]))
    assert got["count"].tolist() == [5]


def test_refusals_of_the_restatement():
    planes, settings, _, _ = hand_case("duplicate", 0)
    for over in ({"dims": 4}, {"dims": 2, "same_class": 1}):
        with pytest.raises(ValueError):
            run_host(planes, tables(), dict(settings, **over))


def test_seam_reach():
    core = np.array([[-INF, 5, -INF, 3], [0.1, INF, 16777216.0, INF], [-INF, INF, -INF, INF]], np.float32)
    reach = D.seam_reach(core, 0.3)
    assert reach.dtype == np.float32 and reach.shape == (3, 4)
    want = np.array([[-INF, np.float32(5.3), -INF, np.float32(3.3)],
                     [np.float32(np.float64(np.float32(0.1)) - 0.3), INF, 16777216.0, INF],
                     [-INF, INF, -INF, INF]], np.float32)
    assert np.array_equal(bits(reach), bits(want))
    # rounded once: float32(0.1) - float32(0.3) in float32 is another number
    assert reach[1, 0] != np.float32(0.1) - np.float32(0.3)
    assert np.array_equal(bits(D.seam_reach(core, 0)), bits(core))
    assert np.array_equal(bits(D.seam_reach(CORE, 0.5)[0]), bits(np.array([-INF, 5.5, -INF, 3.5], np.float32)))
    for bad in (-0.001, -1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="seam"):
            D.seam_reach(core, bad)


def test_seam_settings():
    cd = {"use_3d_nms": True, "nms_iou": 0.25, "use_old_type_nms": False, "cls_nms": True, "use_iou_for_nms": True}
    assert D.seam_settings(cd, 0.5) == {"seam": 0.5, "thresh": 0.25, "old_type": 0, "same_class": 1, "dims": 3}
    cd.update(use_3d_nms=False, use_old_type_nms=True)
    assert D.seam_settings(cd, 1) == {"seam": 1.0, "thresh": 0.25, "old_type": 1, "same_class": 0, "dims": 2}
    assert V.host_merge_nms is D.host_merge_nms and V.seam_reach is D.seam_reach and V.merge_nms_gpu is D.merge_nms_gpu


# ------------------------------------------------------------------ the seeded cases of the GPU tests
def test_random_case_has_what_the_gpu_comparison_needs():
    planes, tab = random_case(3)
    assert tab["tiles"].tolist() == [8, 5] and planes["proposal"].shape == (13, 70)
    assert (1, 1) not in set(zip(tab["iy"][:8].tolist(), tab["ix"][:8].tolist()))  # the hole in the adjacency
    assert tab["iy"][8:].tolist() == [0] * 5 and tab["ix"][8:].tolist() == list(range(5))
    xy = planes["box"][..., 0:2]
    for t in range(13):  # every centre within 0.5 m of one of its tile's cuts, on the 1/64 grid
        c = int(planes["count"][t])
        assert 65 <= c <= 70
        cuts = tab["core"][t][np.isfinite(tab["core"][t])]
        axes = np.array([k // 2 for k in range(4) if np.isfinite(tab["core"][t][k])])
        dist = np.abs(xy[t, :c][:, axes] - cuts[None]).min(1)
        assert (dist <= 0.5).all() and np.array_equal(xy[t, :c] * 64, np.round(xy[t, :c] * 64))
    for settings in (SETTINGS, dict(SETTINGS, dims=2, same_class=0), dict(SETTINGS, old_type=1)):
        info = {}
        got = run_host(planes, tab, settings, info=info)
        for s in (0, 1):
            assert info["rounds"][s] >= 3, info           # a chain of suppressions at least three deep
            assert info["kept_guests"][s] >= 1, info
            assert info["dropped_owned"][s] >= 1, info
            assert info["most_candidates"][s] > 64, info  # one tile's candidates cross a wave
        assert max(info["most_above"]) > 4, info  # some row has more partners above it than the kernel records
        base = D.host_merge(planes, tab["first"], tab["tiles"], tab["core"])
        assert (got["count"] != base["count"]).any()


def test_large_case_has_more_candidates_than_a_workgroup_has_threads():
    planes, tab = large_case(0)
    assert tab["tiles"].tolist() == [16] and int(planes["count"].sum()) > 1024
    inside = sum(int(ST.in_box(planes["box"][t, :planes["count"][t], 0:2], tab["reach"][t]).sum()) for t in range(16))
    assert inside > 1024
    info = {}
    run_host(planes, tab, SETTINGS, info=info)
    assert info["rounds"][0] >= 3 and info["pairs"][0] >= 100


# ------------------------------------------------------------------ the store and the front end
def test_tile_store_remembers_tile_and_overlap():
    g = np.random.default_rng(3)
    clouds = [(g.random((400, 3)) * [10, 5, 3]).astype(np.float32)]
    store = ST.TileStore.from_store(SC.ScanStore(clouds, None, "scannet"), (4.0, 3.0), overlap=1.0)
    assert store.tile == (4.0, 3.0) and store.overlap == 1.0
    assert ST.TileStore.from_store(SC.ScanStore(clouds, None, "scannet"), 6, overlap=0.5).tile == (6.0, 6.0)
    reach = D.seam_reach(store.core, store.overlap / 2)
    assert (reach[:, 0] <= store.core[:, 0]).all() and (reach[:, 1] >= store.core[:, 1]).all()
    assert (store.window[:, 0] <= reach[:, 0]).all() and (reach[:, 1] <= store.window[:, 1]).all()  # inside the window


def _tool():
    spec = importlib.util.spec_from_file_location("detect_tool", os.path.join(ROOT, "tools", "detect.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tool_flags():
    tool = _tool()
    flags = tool.parser().parse_args(["a.npy", "--tile", "8", "--seam-nms"])
    assert flags.seam_nms is True and flags.seam is None and tool.seam_flags(flags) == {"seam_nms": True, "seam": None}
    flags = tool.parser().parse_args(["a.npy", "--tile", "8", "6", "--seam-nms", "--seam", "0.75"])
    assert tool.seam_flags(flags) == {"seam_nms": True, "seam": 0.75}
    assert tool.seam_flags(tool.parser().parse_args(["a.npy", "--tile", "8"])) == {}
    for argv in (["a.npy", "--seam-nms"], ["a.npy", "--tile", "8", "--seam", "0.5"],
                 ["a.npy", "--tile", "8", "--seam-nms", "--seam", "-1"]):
        with pytest.raises(SystemExit):
            tool.seam_flags(tool.parser().parse_args(argv))
