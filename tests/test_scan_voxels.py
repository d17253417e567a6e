"""CPU tests of the voxel downsample: host_voxels against a brute-force dict loop, the face / zero /
duplicate / tie rows of the hand-made scan, idempotence of `first`, the refusals, a host-only VoxelStore
(fields, lazy rows, floors, on into TileStore) and the new flags of tools/detect.py."""
import importlib
import importlib.util
import math
import os

import numpy as np
import pytest

import scan_voxel_cases as cases
from conftest import ROOT, load_pkg
from scan_voxel_cases import EDGE, EDGE_VOXEL, KEEPS

load_pkg()
SC = importlib.import_module("3dioumatch_amd.votenet.scan_data")
ST = importlib.import_module("3dioumatch_amd.votenet.scan_tiles")
SV = importlib.import_module("3dioumatch_amd.votenet.scan_voxels")
V = importlib.import_module("3dioumatch_amd.votenet")


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def brute_force(cloud, voxel, keep):
    """The contract written out row by row in Python floats (IEEE float64): a dict from the cell to
    its smallest (rank, index)."""
    v = SV.voxel_sizes(voxel)
    best = {}
    for i, row in enumerate(cloud):
        p = [float(row[a]) for a in range(3)]
        c = tuple(math.floor(p[a] / v[a]) for a in range(3))
        assert all(abs(x) < 1 << 20 for x in c)
        key = ((c[2] + (1 << 20)) << 42) | ((c[1] + (1 << 20)) << 21) | (c[0] + (1 << 20))
        if keep == "first":
            rank = i
        else:
            d = [p[a] - (float(c[a]) + 0.5) * v[a] for a in range(3)]
            d2 = np.float32((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
            rank = (int(d2.view(np.uint32)) << 32) | i
        if key not in best or rank < best[key][0]:
            best[key] = (rank, i)
    return np.array(sorted(i for _, i in best.values()), np.int32)


SMALL = [("edge", 0), ("anisotropic", 0)] + [("boundary", s) for s in range(7)]  # the boundary scans up to 1025 rows


@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("case,scan", SMALL)
def test_host_voxels_is_the_dict_loop(case, scan, keep):
    got = cases.kept(case, keep)[scan]
    want = brute_force(cases.clouds(case)[scan], cases.voxel(case), keep)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert (np.diff(got) > 0).all()  # the scan's own order


def test_the_edge_rows_land_as_stated():
    cloud = cases.edge_cloud()
    cells = SV.voxel_cells(cloud, EDGE_VOXEL)
    assert cells.dtype == np.int64 and cells.shape == (len(cloud), 3)
    assert cells[EDGE["face"]].tolist() == [1, 0, 0]            # on a face: the upper cell
    assert cells[EDGE["below_face"]].tolist() == [0, 0, 0]
    assert cells[EDGE["neg_face"]].tolist() == [-1, 0, 0]
    assert cells[EDGE["above_neg_face"]].tolist() == [-1, 0, 0]
    assert cells[EDGE["neg_zero"]].tolist() == cells[EDGE["pos_zero"]].tolist() == [0, 2, 0]  # both zeros: cell 0
    assert np.signbit(cloud[EDGE["neg_zero"], 0]) and not np.signbit(cloud[EDGE["pos_zero"], 0])
    assert cells[EDGE["far_pos"]].tolist() == [4000, -4001, 0] and cells[EDGE["far_neg"]].tolist() == [-4001, 4000, 0]
    crowd = range(EDGE["crowd"], EDGE["crowd"] + cases.CROWD)
    assert (cells[crowd] == [8, 8, 2]).all()
    keys = SV.voxel_keys(cells)
    assert keys.dtype == np.int64 and (keys >= 0).all()
    assert keys[EDGE["face"]] == ((1 << 20) << 42) | ((1 << 20) << 21) | ((1 << 20) + 1)
    assert len(set(keys.tolist())) == 10

    first, nearest = (set(cases.kept("edge", k)[0].tolist()) for k in KEEPS)
    assert len(first) == len(nearest) == 10
    both = ("face", "below_face", "neg_zero", "twin_a", "far_pos", "far_neg")
    for kept in (first, nearest):
        assert all(EDGE[n] in kept for n in both)
        assert EDGE["twin_b"] not in kept and EDGE["pos_zero"] not in kept  # equal d2: the lower index
    # x = -0.25 and the float32 above it share cell -1; the second is the closer to its centre
    assert EDGE["neg_face"] in first and EDGE["above_neg_face"] not in first
    assert EDGE["above_neg_face"] in nearest and EDGE["neg_face"] not in nearest
    assert EDGE["crowd"] in first and EDGE["mirror_first"] in first and EDGE["centre_first"] in first
    # equal d2 of the mirrored pair: the lower index; the row on the centre has d2 == 0
    assert EDGE["mirror_lo"] in nearest and EDGE["mirror_hi"] not in nearest and EDGE["mirror_first"] not in nearest
    assert EDGE["centre"] in nearest and EDGE["centre_first"] not in nearest
    ranks = SV.voxel_ranks(cloud, cells, EDGE_VOXEL, "nearest")
    assert ranks[EDGE["centre"]] == EDGE["centre"]  # bits(0.0) << 32 | index
    assert ranks[EDGE["mirror_lo"]] >> np.uint64(32) == ranks[EDGE["mirror_hi"]] >> np.uint64(32)
    assert int(ranks[EDGE["mirror_lo"]] >> np.uint64(32)) == int(np.float32(0.0625 ** 2).view(np.uint32))
    d2 = (ranks[list(crowd)] >> np.uint64(32)).astype(np.uint32).view(np.float32)
    assert EDGE["crowd"] + int(np.argmin(d2)) in nearest and EDGE["crowd"] + int(np.argmin(d2)) != EDGE["crowd"]


def test_all_distinct_keeps_every_row_and_one_cell_keeps_one():
    for keep in KEEPS:
        assert np.array_equal(cases.kept("all_distinct", keep)[0], np.arange(cases.DISTINCT_ROWS))
        assert len(cases.kept("one_cell", keep)[0]) == 1
    assert cases.kept("one_cell", "first")[0].tolist() == [0]


@pytest.mark.parametrize("case", ["edge", "boundary", "anisotropic"])
def test_first_is_idempotent(case):
    clouds = [c[k] for c, k in zip(cases.clouds(case), cases.kept(case, "first"))]
    for c, again in zip(clouds, SV.host_voxels(clouds, cases.voxel(case), "first")):
        assert np.array_equal(again, np.arange(len(c)))


def test_voxel_sizes_and_keep_refusals():
    assert SV.voxel_sizes(0.05) == (0.05, 0.05, 0.05) and SV.voxel_sizes([0.5]) == (0.5, 0.5, 0.5)
    assert SV.voxel_sizes((0.05, 0.1, 0.2)) == (0.05, 0.1, 0.2) and SV.voxel_sizes(np.float32(2)) == (2.0, 2.0, 2.0)
    for bad in (0.0, -1.0, np.nan, np.inf, (1.0, 2.0), (1.0, 2.0, 3.0, 4.0), (1.0, 0.0, 1.0), (1.0, 1.0, -np.inf), [],
                "small", None):
        with pytest.raises(ValueError, match="voxel"):
            SV.voxel_sizes(bad)
    cloud = np.zeros((4, 3), np.float32)
    for keep in ("centroid", "", None, 0):
        with pytest.raises(ValueError, match="keep"):
            SV.host_voxels([cloud], 1.0, keep)
    store = SC.ScanStore([cloud], None)
    with pytest.raises(ValueError, match="voxel"):
        SV.VoxelStore.from_store(store, 0.0)
    with pytest.raises(ValueError, match="keep"):
        SV.VoxelStore.from_store(store, 1.0, keep="mean")
    with pytest.raises(TypeError):
        SV.VoxelStore()


def test_a_cell_out_of_range_names_its_scan():
    ok = np.array([[1048575.5, -1048575.0, 0.0], [0.0, 0.0, 0.0]], np.float32)  # cells 2^20 - 1 and -(2^20 - 1)
    assert [len(k) for k in SV.host_voxels([ok], 1.0)] == [2]
    assert SV.voxel_cells(ok, 1.0)[0].tolist() == [1048575, -1048575, 0]
    for bad_value in (1048576.0, -1048575.5, 3e6):
        bad = ok.copy()
        bad[1, 2] = bad_value
        with pytest.raises(ValueError, match=r"beyond 2\^20 cells.*: far \(1\)$"):
            SV.host_voxels([ok, bad, ok], 1.0, names=["near", "far", "nearer"])
        with pytest.raises(ValueError, match=r"scan 1 \(1\)"):
            SV.host_voxels([ok, bad], 1.0, keep="nearest")
        with pytest.raises(ValueError, match="cells out of range"):
            SV.voxel_keys(SV.voxel_cells(bad, 1.0))
    assert len(SV.host_voxels([bad], 4.0)[0]) == 2  # the same rows at a coarser voxel are in range
    with pytest.raises(ValueError, match=r"far \(1\)"):
        SV.VoxelStore.from_store(SC.ScanStore([ok, bad], None, names=["near", "far"]), 1.0)


@pytest.mark.parametrize("keep", KEEPS)
def test_a_host_only_voxel_store(keep):
    clouds = cases.clouds("boundary", 6)[:7] + cases.clouds("edge", 6)
    names = ["s%d" % i for i in range(8)]
    voxel = cases.BOUNDARY_VOXEL
    parent = SC.ScanStore(clouds, None, "scannet", names=names)
    store = SV.VoxelStore.from_store(parent, voxel, keep=keep)
    want = SV.host_voxels(clouds, voxel, keep)
    assert isinstance(store, SC.ScanStore) and not isinstance(store, ST.TileStore)
    assert store.dev is None and store.device is None and len(store) == 8
    assert store.names == names and store.names is not parent.names
    assert store.source_store is parent and store.voxel == (voxel,) * 3 and store.keep == keep
    assert store.columns == 6 and store.dataset == "scannet"
    assert store.count.dtype == np.int32 and store.count.tolist() == [len(k) for k in want]
    assert store.offset.dtype == np.int64
    assert store.offset.tolist() == np.concatenate([[0], np.cumsum(store.count)[:-1]]).tolist()
    assert store.source.dtype == np.int32 and np.array_equal(store.source, np.concatenate(want))
    assert store._clouds is None and store._floor is None  # filled at first use
    for s, k in enumerate(want):
        assert np.array_equal(bits(store.clouds[s]), bits(clouds[s][k]))
    plain = SC.ScanStore([c[k] for c, k in zip(clouds, want)], None, "scannet", names=names)
    assert store.floor.dtype == np.float32 and np.array_equal(bits(store.floor), bits(plain.floor))
    assert store.clouds is store.clouds and store.floor is store.floor
    got = SC.ScanLoader(store, 64, use_color=True, seed=3).host_batch([0, 7, 3], counter=2)
    ref = SC.ScanLoader(plain, 64, use_color=True, seed=3).host_batch([0, 7, 3], counter=2)
    assert np.array_equal(bits(got["point_clouds"]), bits(ref["point_clouds"]))
    if keep == "first":  # downsampling the result again returns it
        again = SV.VoxelStore.from_store(store, voxel)
        assert again.source_store is store and np.array_equal(again.count, store.count)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(again.clouds, store.clouds))


def test_tiling_comes_after():
    clouds = [cases.anisotropic(3)]
    parent = SC.ScanStore(clouds, None, "scannet", names=["room"])
    store = SV.VoxelStore.from_store(parent, cases.ANISO_VOXEL)
    tiles = ST.TileStore.from_store(store, (2.5, 2.5), overlap=0.5)
    assert tiles.source is store and tiles.parent_names == ["room"] and tiles.tiles.tolist() == [4]
    kept = clouds[0][cases.kept("anisotropic", "first")[0]]
    grid = ST.tile_grid(ST.host_bounds([kept]), (2.5, 2.5), 0.5)
    _, crops = ST.host_tiles([kept], grid)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(tiles.clouds, crops))
    with pytest.raises(ValueError, match="TileStore"):
        SV.VoxelStore.from_store(tiles, 0.1)
    for other in (clouds, None, "store"):
        with pytest.raises(ValueError, match="ScanStore"):
            SV.VoxelStore.from_store(other, 0.1)


def test_exports_and_table_sizes():
    assert V.VoxelStore is SV.VoxelStore and V.host_voxels is SV.host_voxels
    L = importlib.import_module("3dioumatch_amd._lib")
    for name in ("scene_scan_voxel_slots", "scene_scan_voxel_mark", "scene_scan_voxel_count", "scene_scan_voxel_gather"):
        assert name in L._LOADER_SIGNATURES and name not in L.EXPORTS and hasattr(L.lib, name)
    for n in (1, 2, 3, 4, 5, 63, 64, 65, 4096, 4097, 65536, 131073, (1 << 30) - 1):  # a host function
        slots = L.lib.scene_scan_voxel_slots(n)
        assert slots == SV.voxel_slots(n) and slots >= max(2, 2 * n) and slots & (slots - 1) == 0 and slots < 4 * n + 2
    for n in (0, -1, 1 << 30):
        assert L.lib.scene_scan_voxel_slots(n) == SV.voxel_slots(n) == 0
    assert SV.CELL_LIMIT == 1 << 20 and ST.SEGMENT == 65536


# ------------------------------------------------------------------ tools/detect.py
def _tool():
    spec = importlib.util.spec_from_file_location("tools_detect_voxel", os.path.join(ROOT, "tools", "detect.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_detect_tool_voxel_flags():
    tool = _tool()
    flags = tool.parser().parse_args(["a.npy"])
    assert flags.voxel is None and tool.voxeling(flags) is None  # no --voxel: the path as it was
    assert tool.voxeling(tool.parser().parse_args(["a.npy", "--voxel", "0.05"])) == ((0.05, 0.05, 0.05), "first")
    flags = tool.parser().parse_args(["--voxel", "0.05", "0.1", "0.2", "--voxel-keep", "nearest", "--tile", "8", "--",
                                      "a.npy"])
    assert tool.voxeling(flags) == ((0.05, 0.1, 0.2), "nearest") and tool.tiling(flags) == ((8.0, 8.0), 1.0, 1)
    with pytest.raises(SystemExit, match="one or three"):
        tool.voxeling(tool.parser().parse_args(["--voxel", "0.05", "0.1"]))
    for bad in ("0", "-0.1", "nan", "inf"):
        with pytest.raises(SystemExit, match="> 0"):
            tool.voxeling(tool.parser().parse_args(["a.npy", "--voxel", bad]))
    with pytest.raises(SystemExit, match="goes with --voxel"):
        tool.voxeling(tool.parser().parse_args(["a.npy", "--voxel-keep", "nearest"]))
    with pytest.raises(SystemExit):  # argparse's own: not one of the choices
        tool.parser().parse_args(["a.npy", "--voxel", "1", "--voxel-keep", "mean"])
